"""``Simulation``: the reference's driver for the atmosphere path, device-backed.

Mirrors ``maria.sim.Simulation`` (sim/simulation.py:66-272) and the atmosphere
mixin (sim/atmosphere.py:24-84) for what BASELINE.json's north star covers:
``Simulation(instrument, plans, site, atmosphere="2d", atmosphere_kwargs=...)``
and ``.run(units)`` returning one ``TOD`` per plan.  The CMB, map and noise mixins
and unit conversions other than pW are follow-on rows and say so.
"""

from __future__ import annotations

import logging
import time as ttime

import numpy as np

from . import _tod_args
from .atmosphere import Atmosphere
from .instrument import Instrument, Site

logger = logging.getLogger("maria")

MIN_ELEVATION_WARN = 10  # sim/observation.py
MIN_ELEVATION_ERROR = 5
HALF_PI_F32 = np.float32(np.pi / 2)


class PointingError(Exception):
    """maria/errors/__init__.py:8."""


class Coordinates:
    """az/el pointing of a boresight or of detectors around it (host-side numpy).

    The slice of ``maria.coords.Coordinates`` the atmosphere set-up needs:
    ``downsample`` (coordinates.py:286-304), ``broadcast`` to detector offsets in
    float32 like jax does (coordinates.py:378-386, transforms.py:10-29) and the
    unit-height ground projection (coordinates.py:333-349)."""

    def __init__(self, t, az, el, offsets=None):
        self.t = np.asarray(t, float)
        self._baz, self._bel = np.asarray(az, float), np.asarray(el, float)
        self.offsets = None if offsets is None else np.atleast_2d(np.asarray(offsets, float))
        self._azel = None

    def _pointing(self):
        if self.offsets is None:
            return self._baz, self._bel
        if self._azel is None:
            f32 = np.float32
            dx, dy = self.offsets[:, 0, None].astype(f32), self.offsets[:, 1, None].astype(f32)
            r = np.sqrt(dx * dx + dy * dy)
            p = np.arctan2(-dx, -dy)
            a = self._bel[None].astype(f32) - HALF_PI_F32
            a_re, a_im = np.sin(r) * np.cos(p), np.cos(r)
            re = a_re * np.cos(a) - a_im * np.sin(a)
            im = a_re * np.sin(a) + a_im * np.cos(a)
            self._azel = (np.arctan2(np.sin(r) * np.sin(p), re) + self._baz[None].astype(f32), np.arcsin(im))
        return self._azel

    @property
    def az(self):
        return self._pointing()[0]

    @property
    def el(self):
        return self._pointing()[1]

    @property
    def shape(self):
        return self.az.shape

    def downsample(self, timestep):
        ds_t = np.arange(self.t.min(), self.t.max(), timestep)
        return Coordinates(ds_t, np.interp(ds_t, self.t, self._baz), np.interp(ds_t, self.t, self._bel))

    def broadcast(self, offsets):
        return Coordinates(self.t, self._baz, self._bel, offsets=offsets)

    def project_unit(self):
        """(cos az / tan el, sin az / tan el) [.., Ta, 2]: ``project(z=1)`` from the origin."""
        az, el = self._pointing()
        tan_el = np.tan(el)
        return np.stack([np.cos(az) / tan_el, np.sin(az) / tan_el], axis=-1).astype(np.float64)


def sky_transform_stack(t, latitude_deg, longitude_deg):
    """[T, 3, 3] float64 with ``xyz(az, el) @ M[t] = xyz(ra, dec)``: the per-sample transform
    coords/coordinates.py:184-236 fits to astropy's AltAz -> ICRS at fiducial times and
    interpolates.  astropy is not available to this package, so the rotation is the
    textbook one -- horizon to hour angle/declination at the site's latitude, then the local
    sidereal angle (GMST of IAU 1982 + longitude) -- without precession, nutation, aberration
    or refraction: coordinates "of date", self-consistent within a simulation.  A caller with
    astropy hands its own stack to ``mrx_map_sample``."""
    t = np.asarray(t, float)
    lat = np.radians(latitude_deg)
    days = t / 86400.0 + 2440587.5 - 2451545.0
    lst = np.radians(15.0 * ((18.697374558 + 24.06570982441908 * days) % 24.0) + longitude_deg)
    A = np.array([[-np.sin(lat), 0.0, np.cos(lat)], [0.0, -1.0, 0.0], [np.cos(lat), 0.0, np.sin(lat)]])  # (N, E, U) -> hour-angle frame
    B = np.zeros((len(t), 3, 3))
    B[:, 0, 0], B[:, 0, 1] = np.cos(lst), np.sin(lst)
    B[:, 1, 0], B[:, 1, 1] = np.sin(lst), -np.cos(lst)
    B[:, 2, 2] = 1.0
    return A[None] @ B


class Plan:
    """Time-ordered boresight in the az/el frame (``maria.plan.Plan``'s ``time``,
    ``phi``, ``theta``; other frames need astropy and stay with maria's front end)."""

    def __init__(self, time, az, el, roll=0.0):
        self.time = np.asarray(time, float)
        self.phi, self.theta = np.asarray(az, float), np.asarray(el, float)
        self.frame, self.roll = "az/el", roll
        if self.time.ndim != 1 or self.phi.shape != self.time.shape or self.theta.shape != self.time.shape:
            raise ValueError("time, az and el must be one-dimensional and of equal length")

    @classmethod
    def daisy(cls, start_time=0.0, duration=60.0, sample_rate=50.0, scan_center=(45.0, 60.0), radius=0.5, speed=0.5):
        """plan/plan.py:55-140 with ``scan_pattern="daisy"`` in az/el, degrees."""
        from .synthetic import daisy_scan

        t = np.arange(start_time, start_time + duration, 1.0 / sample_rate)  # plan.py:83
        az, el = daisy_scan(t, radius, speed, scan_center[0], scan_center[1])
        return cls(t, az, el)

    @classmethod
    def back_and_forth(cls, start_time=0.0, duration=60.0, sample_rate=50.0, scan_center=(45.0, 60.0), throw=2.0, speed=1.0, accel=2.0):
        """A constant-elevation scan in az/el, degrees: the azimuth sweeps ``scan_center[0]`` -+ ``throw`` at ``speed``
        (degrees of azimuth a second) and turns round beyond them at ``accel`` (``subscans.back_and_forth``); the elevation
        stays at ``scan_center[1]``."""
        from .subscans import back_and_forth

        t = np.arange(start_time, start_time + duration, 1.0 / sample_rate)
        az = np.radians(scan_center[0] + back_and_forth(t - start_time, throw, speed, accel))
        return cls(t, az, np.full(t.shape, np.radians(scan_center[1])))

    @property
    def duration(self):
        return float(self.time[-1] - self.time[0])


class Observation:
    """sim/observation.py:27-100."""

    def __init__(self, instrument, plan, site, atmosphere=None, atmosphere_kwargs={}):
        self.instrument, self.plan, self.site = instrument, plan, site
        self.boresight = Coordinates(plan.time, plan.phi, plan.theta)
        c, s = np.cos(np.radians(plan.roll)), np.sin(np.radians(plan.roll))
        self.coords = self.boresight.broadcast(instrument.dets.offsets @ np.array([[c, -s], [s, c]]).T)
        # the elevation checks of observation.py:61-71, on the hull detectors (the extremes)
        el_min = float(self.boresight.downsample(1.0).broadcast(instrument.dets.outer().offsets).el.min()) if len(plan.time) > 1 else float(plan.theta.min())
        el_min = min(el_min, float(plan.theta.min()))
        if el_min < np.radians(MIN_ELEVATION_WARN):
            logger.warning(f"Some detectors come within {MIN_ELEVATION_WARN} degrees of the horizon (el_min = {np.degrees(el_min):.01f} deg)")
        if el_min <= np.radians(MIN_ELEVATION_ERROR):
            raise PointingError(f"Some detectors come within {MIN_ELEVATION_ERROR} degrees of the horizon (el_min = {np.degrees(el_min):.01f} deg)")
        if atmosphere:
            self.atmosphere_kwargs = atmosphere_kwargs
            if isinstance(atmosphere, Atmosphere):
                self.atmosphere = atmosphere
            else:
                self.atmosphere = Atmosphere(model=atmosphere, timestamp=float(plan.time.mean()), region=site.region, altitude=site.altitude, **atmosphere_kwargs)
        self.loading = {}


class TOD:
    """The slice of ``maria.tod.TOD`` this path fills: ``data`` (dict of [ndet, nt]
    float32 arrays, numpy or device tensors), ``dets``, ``coords``, ``units``, ``metadata``.  ``flags``: None, or a
    [ndet, nt] uint8 device tensor whose nonzero entries mark samples the mappers give no weight (``flag_glitches``,
    ``fix_jumps``, ``filter_subscans``, ``cut``)."""

    def __init__(self, data, dets, coords, units="pW", metadata=None, flags=None):
        self.data, self.dets, self.coords, self.units = data, dets, coords, units
        self.metadata = metadata or {}
        self.flags = flags

    @property
    def fields(self):
        return list(self.data)

    @property
    def signal(self):
        return sum(self.data.values())

    @property
    def time(self):
        return self.coords.t

    def psd(self, nperseg=None, field=None, ctx=None, device="cuda:0"):
        """The Welch spectrum of every detector's row of ``field`` (default: the signal, the sum of the fields) on the
        device: ``(f, psd)``, maria_amd.noise_estimate.welch."""
        import torch

        from .noise_estimate import welch

        fields = [self.data[field]] if field is not None else list(self.data.values())
        x = None
        for v in fields:
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            dev = v.device if v.is_cuda else torch.device(device)
            x = v.to(dev, torch.float32).clone() if x is None else x.add_(v.to(x.device, torch.float32))
        t = np.asarray(self.coords.t, float)
        fs = (t.size - 1) / (t[-1] - t[0])
        return welch(x.contiguous(), fs, nperseg=nperseg, ctx=ctx)

    def fit_noise(self, nperseg=None, field=None, f_min=None, f_max=None, n_bins=32, ctx=None, device="cuda:0"):
        """Per detector, the noise law fitted to :meth:`psd` (maria_amd.noise_estimate.fit_noise): a dict of ``white``,
        ``knee``, ``alpha``, ``sigma`` and ``knee_at_floor`` tensors."""
        from .noise_estimate import fit_noise

        f, p = self.psd(nperseg=nperseg, field=field, ctx=ctx, device=device)
        return fit_noise(f, p, f_min=f_min, f_max=f_max, n_bins=n_bins)

    def downsample(self, q, taps=None, ctx=None, device="cuda:0"):
        """A new TOD at 1 / q of the sample rate (q = 2 .. 32): every field low-passed and decimated on the device by
        maria_amd.downsample.decimate (``taps`` None: scipy.signal.decimate's FIR for q), one field at a time, into
        float32 device tensors; the boresight picked at every q-th sample (it is smooth, and picking keeps azimuth wraps
        out of the filter), output sample j at time t[j q].  ``dets``, ``units`` and ``metadata`` are carried over and
        ``metadata["downsample"]`` records the factor, the tap count and the new sample rate.  The pW <-> K_RJ
        calibrator is NOT carried over (it closes over full-rate tables): ``to()`` on the result raises
        NotImplementedError, so convert units first.  ``flags`` become ``flagging.downsample_flags(flags, q)``: an output is
        flagged if any input within q samples of it is.  This TOD is left as it is."""
        import torch

        from ._lib import Context
        from .downsample import MAX_FACTOR, MIN_FACTOR, decimate, design_taps, upload_taps

        if int(q) != q or not MIN_FACTOR <= int(q) <= MAX_FACTOR:
            raise ValueError(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
        q = int(q)
        h = design_taps(q) if taps is None else np.ascontiguousarray(_tod_args.to_numpy(taps), np.float64)
        data, d_taps = {}, {}  # the taps go to a device once, and one context serves every field
        for name, v in self.data.items():
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            dev = v.device if v.is_cuda else torch.device(device)
            x = v.to(dev, torch.float32)
            if x.dim() == 2 and x.shape[1] > 1 and x.stride(1) != 1:
                x = x.contiguous()
            if ctx is None:
                ctx = Context(dev.index or 0)
                ctx.set_stream(torch.cuda.current_stream(dev))
            if dev not in d_taps:
                d_taps[dev] = upload_taps(h, dev)
            data[name] = decimate(x, q, taps=h, ctx=ctx, device_taps=d_taps[dev])
        c = self.coords
        t = np.asarray(c.t, float)
        coords = Coordinates(t[::q], c._baz[::q], c._bel[::q], offsets=c.offsets)
        metadata = dict(self.metadata)
        rate = (t.size - 1) / (t[-1] - t[0]) / q if t.size > 1 else float("nan")
        metadata["downsample"] = {"factor": q, "n_taps": int(h.size), "sample_rate": float(rate)}
        flags = None
        if self.flags is not None:
            from .flagging import downsample_flags

            flags = downsample_flags(self.flags, q)
        return TOD(data=data, dets=self.dets, coords=coords, units=self.units, metadata=metadata, flags=flags)

    def demodulate(self, hwp=None, q=None, taps_t=None, taps_p=None, ctx=None, device="cuda:0"):
        """A new TOD at 1 / q of the sample rate whose rows are the T, Q and U series of every detector behind a rotating
        half-wave plate (maria_amd.hwp.demodulate): every field locked in against the carrier
        (cos 4 chi, sin 4 chi) and low-passed on the device, one field at a time, into float32 device tensors of
        D + 2 D_pol rows -- the T rows of all D detectors, then the Q rows and then the U rows of the D_pol polarised
        ones (an unpolarised detector carries no polarisation signal).  ``hwp``: the maria_amd.hwp.HWP (None:
        ``metadata["hwp"]``, which the simulation wrote); ``q`` (2 .. 32; None: min(32, hwp.max_factor(...)));
        ``taps_t``, ``taps_p``: the low-passes of T and of Q / U (one of them given serves for both; neither:
        ``hwp.design_taps(sample rate, f_hwp)``).  The
        boresight and the times are picked at every q-th sample, output sample j at time t[j q].  ``dets`` is
        ``hwp.demodulated_detectors(self.dets)``, whose ``stokes_rows()`` the mappers take: a Q row is a detector of angle
        -gamma without I weight, a U row one of angle pi / 4 - gamma; ``coords.offsets`` are repeated to match.  ``units``
        and ``metadata`` are carried over and ``metadata["demodulate"]`` records ``f_hwp``, ``factor``, ``n_taps``,
        ``sample_rate`` and the row ranges ``rows`` of T, Q and U.  The pW <-> K_RJ calibrator is NOT carried over: ``to()``
        on the result raises NotImplementedError, so convert units first.  ``flags`` become
        ``flagging.downsample_flags(flags, q)``, repeated for the Q / U rows.  This TOD is left as it is.  Its place in
        the chain is downsample's, after deconvolve_time_constants and instead of downsample: a detector lag attenuates and
        delays the 4 f carrier, which rotates Q into U."""
        import torch

        from . import hwp as mhwp
        from ._lib import Context
        from .downsample import MAX_FACTOR, MIN_FACTOR

        if "demodulate" in self.metadata or "downsample" in self.metadata:
            raise ValueError("demodulate takes the TOD at the rate the half-wave plate modulated it: this one is already reduced")
        if hwp is None:
            if "hwp" not in self.metadata:
                raise ValueError('no hwp given and no metadata["hwp"]: this TOD was not simulated behind a half-wave plate')
            hwp = mhwp.HWP.from_metadata(self.metadata["hwp"])
        t = np.asarray(self.coords.t, float)
        if t.size < 2:
            raise ValueError("demodulate needs at least two samples to know the sample rate")
        fs = (t.size - 1) / (t[-1] - t[0])
        if q is None:
            q = min(MAX_FACTOR, mhwp.max_factor(fs, hwp.frequency))
        if int(q) != q or not MIN_FACTOR <= int(q) <= MAX_FACTOR:
            raise ValueError(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
        q = int(q)
        host = lambda h: np.ascontiguousarray(_tod_args.to_numpy(h), np.float64)  # noqa: E731
        if taps_t is None and taps_p is None:
            ht = hp = mhwp.design_taps(fs, hwp.frequency)
        else:  # one of them given serves for both
            hp = host(taps_t if taps_p is None else taps_p)
            ht = hp if taps_t is None else host(taps_t)
        c = mhwp.carrier(hwp.angle(t))
        D = self.dets.n
        pol = mhwp.polarized_rows(self.dets)
        Dp = int(pol.size)
        T_out = (t.size + q - 1) // q
        data, d_carrier = {}, {}  # the carrier goes to a device once, and one context serves every field
        for name, v in self.data.items():
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            dev = v.device if v.is_cuda else torch.device(device)
            x = v.to(dev, torch.float32)
            if x.dim() == 2 and x.shape[1] > 1 and x.stride(1) != 1:
                x = x.contiguous()
            if ctx is None:
                ctx = Context(dev.index or 0)
                ctx.set_stream(torch.cuda.current_stream(dev))
            if dev not in d_carrier:
                d_carrier[dev] = torch.as_tensor(c).to(dev)
            y = torch.empty((D + 2 * Dp, T_out), dtype=torch.float32, device=dev)
            if Dp == D:  # every detector has Q and U rows: the three outputs are the three blocks of the field
                mhwp.demodulate(x, d_carrier[dev], q, ht, hp, ctx=ctx, out=(y[:D], y[D:2 * D], y[2 * D:]))
            else:
                _, yq, yu = mhwp.demodulate(x, d_carrier[dev], q, ht, hp, ctx=ctx, out=(y[:D], *torch.empty((2, D, T_out), dtype=torch.float32, device=dev)))
                rows = torch.as_tensor(pol).to(dev)
                y[D:D + Dp] = yq.index_select(0, rows)
                y[D + Dp:] = yu.index_select(0, rows)
            data[name] = y
        idx = np.concatenate([np.arange(D), pol, pol])
        cd = self.coords
        coords = Coordinates(t[::q], cd._baz[::q], cd._bel[::q], offsets=None if cd.offsets is None else cd.offsets[idx])
        metadata = dict(self.metadata)
        metadata["demodulate"] = {"f_hwp": hwp.frequency, "factor": q, "n_taps": int(hp.size), "sample_rate": float(fs / q),
                                  "rows": {"T": (0, D), "Q": (D, D + Dp), "U": (D + Dp, D + 2 * Dp)}}
        flags = None
        if self.flags is not None:
            from .flagging import downsample_flags

            low = downsample_flags(torch.as_tensor(self.flags), q)
            flags = low.index_select(0, torch.as_tensor(idx).to(low.device))
        return TOD(data=data, dets=mhwp.demodulated_detectors(self.dets), coords=coords, units=self.units, metadata=metadata, flags=flags)

    def remove_hwpss(self, harmonics=(1, 2), hwp=None, **regress_kw):
        """A new TOD with the half-wave plate's synchronous signal fitted and removed: ``TOD.regress`` on the templates
        cos k chi, sin k chi of the ``harmonics`` k (at most 4: regress takes 8 templates), ``hwp.harmonic_templates``.
        ``hwp`` None: ``metadata["hwp"]``; ``regress_kw``: ``model``, ``into``, ``min_hits``, ``rcond``, ``ctx``,
        ``device``.  It runs at the full rate, before ``demodulate``.  Removing harmonic 4 also removes any polarisation
        that is constant in the instrument's frame -- and with it the part of the sky's that happens to be.
        ``metadata["regress"]`` is regress's, and ``metadata["hwpss"]`` records the harmonics."""
        from . import hwp as mhwp

        ks = tuple(harmonics)
        if not 1 <= len(ks) <= mhwp.MAX_HARMONICS:
            raise ValueError(f"harmonics {harmonics}: 1 .. {mhwp.MAX_HARMONICS} of them")
        if hwp is None:
            if "hwp" not in self.metadata:
                raise ValueError('no hwp given and no metadata["hwp"]: this TOD was not simulated behind a half-wave plate')
            hwp = mhwp.HWP.from_metadata(self.metadata["hwp"])
        out = self.regress(mhwp.harmonic_templates(hwp.angle(self.coords.t), ks), **regress_kw)
        out.metadata["hwpss"] = {"harmonics": tuple(int(k) for k in ks)}
        return out

    def flag_glitches(self, n_sigma=6.0, half_window=5, grow=(2, 8), n_fit=4, fill=True, ctx=None, device="cuda:0"):
        """A new TOD with glitches flagged and, with ``fill``, filled (maria_amd.flagging).  Glitches are
        detected on the signal (the sum of the fields): samples further than ``n_sigma`` robust sigmas from the running
        median of 2 * half_window + 1 samples, grown by ``grow = (before, after)`` samples, ORed into any ``flags`` this
        TOD already has.  Every field of the result is a float32 device copy whose flagged samples are replaced by the
        line between the means of the ``n_fit`` unflagged samples either side (no noise is added), so that the
        pre-processing filters do not ring; ``flags`` is the [D, T] uint8 device tensor the mappers take as zero weight, and
        ``metadata["glitches"]`` records the parameters, ``flagged_fraction`` and the per-row ``counts``.  ``dets``,
        ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried over.  This TOD is left as it is."""
        import torch

        from ._lib import Context
        from .flagging import find_glitches, gap_fill

        data, signal, dev = {}, None, None
        for name, v in self.data.items():
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if dev is None:  # the first field's device (a host field: ``device``) takes them all
                dev = v.device if v.is_cuda else torch.device(device)
            data[name] = v.to(dev, torch.float32, copy=True).contiguous()
            signal = data[name].clone() if signal is None else signal.add_(data[name])
        if ctx is None:
            ctx = Context(dev.index or 0)
            ctx.set_stream(torch.cuda.current_stream(dev))
        flags, count = find_glitches(signal, n_sigma=n_sigma, half_window=half_window, grow=grow, ctx=ctx)
        del signal
        if self.flags is not None:
            flags |= torch.as_tensor(self.flags).to(dev, torch.uint8)
            count = (flags != 0).sum(dim=1)
        if fill:
            for x in data.values():
                gap_fill(x, flags, n_fit=n_fit, ctx=ctx)
        metadata = dict(self.metadata)
        counts = count.cpu().numpy().astype(np.int64)
        metadata["glitches"] = {"n_sigma": float(n_sigma), "half_window": int(half_window), "grow": (int(grow[0]), int(grow[1])),
                                "n_fit": int(n_fit), "fill": bool(fill), "flagged_fraction": float(counts.sum() / flags.numel()),
                                "counts": counts}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def fix_jumps(self, window=64, n_sigma=8.0, gap=4, sep=None, grow=(4, 4), min_count=None, model=None, into=None, n_fit=4, fill=True,
                  ctx=None, device="cuda:0"):
        """A new TOD with the jumps of every detector found, taken out and flagged (maria_amd.jumps).  Jumps
        are the peaks of the step statistic of the signal (the sum of the fields, less ``model``): the mean of the
        ``window`` samples after a sample less the mean of those before it, above ``n_sigma`` robust scales of the
        statistic itself and more than ``sep`` (None: window) samples apart.  Samples with nonzero ``flags`` are kept
        out of every mean, so run ``flag_glitches`` first: a 40 sigma spike shifts the statistic by 40 sigma / window
        over window samples.  A jump's height is the same difference of means with the ``gap`` samples either side of
        it left out and the windows clipped at the neighbouring jumps; the steps are subtracted from the field ``into``
        (default: the first; the mappers bin the sum).  A jump with fewer than ``min_count`` (None: window // 2) valid
        samples on a side has no height: it is flagged, counted in ``unfixed`` and left in the data.  The samples within
        ``grow = (before, after)`` of a jump are ORed into the flags and, with ``fill``, every field is filled over the
        new flags by ``flagging.gap_fill`` with ``n_fit``.  ``model``: the expected sky signal, or a drift to keep out of
        the statistic.  Every field of the result is a float32 device copy; ``dets``, ``coords``, ``units`` and the
        pW <-> K_RJ calibrator are carried over; ``metadata["jumps"]`` records the parameters, the per-row ``counts``,
        ``positions`` and ``heights`` (a list of arrays, one a row; 0 for an unfixed jump), ``unfixed`` and
        ``flagged_fraction``.  This TOD is left as it is."""
        import torch

        from . import jumps
        from .flagging import MAX_FIT, _check_grow, gap_fill

        w, g, m = jumps._check_window(window, gap, min_count)
        sep = jumps._check_sep(sep, w)
        grow = _check_grow(grow)
        if int(n_fit) != n_fit or not 1 <= int(n_fit) <= MAX_FIT:
            raise ValueError(f"n_fit {n_fit}: an integer in 1 .. {MAX_FIT}")
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        if model is not None:
            signal.sub_(model)
        row_start, pos, jump_flags, count = jumps.find_jumps(signal, window=w, n_sigma=n_sigma, sep=sep, grow=grow, flags=flags,
                                                             min_count=m, ctx=ctx)
        height, ok = jumps.jump_heights(signal, row_start, pos, w, g, flags=flags, min_count=m, ctx=ctx)
        del signal
        jumps.fix_jumps(data[into], row_start, pos, height, out=data[into], ctx=ctx)
        if flags is not None:
            jump_flags |= flags
        if fill:
            for x in data.values():
                gap_fill(x, jump_flags, n_fit=int(n_fit), ctx=ctx)
        rs, ps, hs = row_start.cpu().numpy(), pos.cpu().numpy().astype(np.int64), height.cpu().numpy()
        metadata = dict(self.metadata)
        metadata["jumps"] = {"window": w, "n_sigma": float(n_sigma), "gap": g, "sep": sep, "grow": grow, "min_count": m, "n_fit": int(n_fit),
                             "fill": bool(fill), "into": into, "counts": count.cpu().numpy().astype(np.int64),
                             "positions": [ps[a:b] for a, b in zip(rs[:-1], rs[1:])], "heights": [hs[a:b] for a, b in zip(rs[:-1], rs[1:])],
                             "unfixed": int((~ok).sum()), "flagged_fraction": float((jump_flags != 0).sum()) / jump_flags.numel()}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=jump_flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def remove_ground(self, n_bins=64, bins=None, model=None, shared=False, min_hits=8, into=None, ctx=None, device="cuda:0"):
        """A new TOD with the scan-synchronous ground pickup removed (maria_amd.ground): per detector, the mean
        of the signal (the sum of the fields) in each of ``n_bins`` uniform bins of the boresight azimuth
        (``ground.azimuth_bins``), subtracted from every sample of the bin.  ``model``: a [D, T] array or tensor of the
        expected sky signal (a previous map sampled back through ``Simulation(map=...)``, or a field of this TOD), taken
        off the signal before the means are formed, so that the subtraction does not eat the sky; without it the template
        holds the sky's own mean in every bin.  Samples with nonzero ``flags`` take no part in the means, and are
        subtracted from like the rest.  ``bins``: any int32 [T] key in -1 .. n_bins - 1 in place of the azimuth bins
        (-1: the sample is left as it is).  ``shared``: one template for all detectors (``ground.shared_template``).
        A (detector, bin) pair with fewer than ``min_hits`` samples gets no template and its samples stay as they are.
        Every field of the result is a float32 device copy; the template is subtracted from the field ``into`` (default:
        the first), the mappers bin the sum.  ``flags``, ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator
        are carried over; ``metadata["ground"]`` records ``n_bins``, ``lo``, ``hi`` (None with ``bins``), ``min_hits``,
        ``shared``, ``empty_bins`` (the (detector, bin) pairs without a template) and the [D, n_bins] float32
        ``template``.  This TOD is left as it is."""
        from . import ground

        n_bins = ground._check_n_bins(n_bins)
        T = int(np.asarray(self.coords.t).size)
        lo = hi = None
        if bins is None:
            bins, lo, hi = ground.azimuth_bins(self.coords._baz, n_bins)
        bins = ground._check_bins(bins, n_bins, T)
        min_hits = _tod_args.check_min_hits(min_hits)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        template, hits, sums = ground.bin_template(signal, bins, n_bins, flags=flags, model=model, min_hits=min_hits, ctx=ctx)
        del signal
        floor = max(int(min_hits), 1)
        if shared:
            template = ground.shared_template(sums, hits, min_hits)
            empty = int((hits.sum(dim=0) < floor).sum()) * int(hits.shape[0])
        else:
            empty = int((hits < floor).sum())
        ground.apply_template(data[into], bins, template, sign=-1, out=data[into], ctx=ctx)
        metadata = dict(self.metadata)
        metadata["ground"] = {"n_bins": n_bins, "lo": lo, "hi": hi, "min_hits": int(min_hits), "shared": bool(shared),
                              "empty_bins": empty, "template": template.cpu().numpy()}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=self.flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def _device_fields(self, model, into, ctx, device):
        """(data, signal, model, flags, into, ctx) for ``remove_ground``, ``regress``, ``remove_common_mode`` and the like: float32
        device copies of the fields, their sum, the model and the flags on the same device."""
        import torch

        from ._lib import Context

        T = int(np.asarray(self.coords.t).size)
        into = self.fields[0] if into is None else into
        if into not in self.data:
            raise ValueError(f"into {into!r}: one of the fields {self.fields}")
        data, signal, dev = {}, None, None
        for name, v in self.data.items():
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if dev is None:  # the first field's device (a host field: ``device``) takes them all
                dev = v.device if v.is_cuda else torch.device(device)
            data[name] = v.to(dev, torch.float32, copy=True).contiguous()
            signal = data[name].clone() if signal is None else signal.add_(data[name])
        if tuple(signal.shape) != (signal.shape[0], T):
            raise ValueError(f"fields of shape {tuple(signal.shape)}: the coordinates have {T} samples")
        if model is not None:
            model = model if isinstance(model, torch.Tensor) else torch.as_tensor(np.asarray(model))
            if tuple(model.shape) != tuple(signal.shape):
                raise ValueError(f"model of shape {tuple(model.shape)}: the fields' {tuple(signal.shape)}")
            model = model.to(dev, torch.float32).contiguous()
        flags = None if self.flags is None else torch.as_tensor(self.flags).to(dev, torch.uint8).contiguous()
        if ctx is None:
            ctx = Context(dev.index or 0)
            ctx.set_stream(torch.cuda.current_stream(dev))
        return data, signal, model, flags, into, ctx

    def regress(self, templates, model=None, into=None, min_hits=8, rcond=1e-10, ctx=None, device="cuda:0"):
        """A new TOD with the [K, T] time ``templates`` (K <= 8; float32, shared by all detectors: ``regress.
        legendre_templates``, ``regress.airmass_template``, anything else) fitted to the signal (the sum of the fields,
        less ``model``) of every detector by least squares and subtracted from the field ``into`` (default: the first; the
        mappers bin the sum) (maria_amd.regress).  Samples with nonzero ``flags`` take no part in the fit,
        and are subtracted from like the rest.  A detector with fewer than max(min_hits, K) samples left, or whose
        templates are degenerate on them (``regress.solve``), is left as it is.  Every field of the result is a float32
        device copy; ``flags``, ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried over;
        ``metadata["regress"]`` records ``n_templates``, ``min_hits``, ``rcond``, the [D, K] float64 ``coefficients`` and
        ``failed_rows``.  This TOD is left as it is."""
        import torch

        from . import regress

        min_hits = _tod_args.check_min_hits(min_hits)
        B = templates if isinstance(templates, torch.Tensor) else torch.as_tensor(np.asarray(templates))
        T = int(np.asarray(self.coords.t).size)
        if B.dim() != 2 or B.shape[1] != T or not 1 <= B.shape[0] <= regress.MAX_TEMPLATES:
            raise ValueError(f"templates must be a [K, {T}] array with K in 1 .. {regress.MAX_TEMPLATES}")
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        B = B.to(signal.device, torch.float32).contiguous()[None]
        N, r, hits = regress.normal_equations(signal, B, flags=flags, model=model, ctx=ctx)
        del signal
        a, ok = regress.solve(N, r, hits, min_hits=min_hits, rcond=rcond)
        regress.apply(data[into], B, a, sign=-1, out=data[into], ctx=ctx)
        metadata = dict(self.metadata)
        metadata["regress"] = {"n_templates": int(B.shape[1]), "min_hits": min_hits, "rcond": float(rcond),
                               "coefficients": a.cpu().numpy(), "failed_rows": np.flatnonzero(~ok.cpu().numpy())}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=self.flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def remove_common_mode(self, groups="band", n_iter=3, poly_order=0, airmass=False, model=None, into=None, min_hits=8, rcond=1e-10,
                           ctx=None, device="cuda:0"):
        """A new TOD with the common mode removed (maria_amd.regress.fit_common_mode): per group of
        detectors the gain-weighted mean of the signal (the sum of the fields, less ``model``) sample by sample, every
        detector fitted to [1, common mode, further templates] by least squares, the fit subtracted from the field
        ``into`` (default: the first), the constant included.  ``groups``: "band" (``dets.band_index``), None (one group)
        or an integer array, -1 leaving a detector out and as it is (at most 16 groups).  Further templates: the Legendre
        polynomials P_1 .. P_poly_order of the time axis and, with ``airmass``, 1 / sin(elevation) less its mean.  Mean
        and fit are iterated ``n_iter`` times, the gains of one fit weighting the next mean.  ``model``: the expected sky
        signal, kept out of mean and fit.  Samples with nonzero ``flags`` take part in neither and are subtracted from
        like the rest; a detector that cannot be fitted (``regress.solve``) is left as it is.  Every field of the result
        is a float32 device copy; ``flags``, ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried
        over; ``metadata["common_mode"]`` records ``n_groups``, ``n_iter``, ``poly_order``, ``airmass``, ``min_hits``,
        ``rcond``, the [D] ``gains`` and ``offsets``, the [D, K] ``coefficients``, the [G, T] float32 ``common_mode``
        and ``failed_rows``.  This TOD is left as it is."""
        from . import regress

        min_hits = _tod_args.check_min_hits(min_hits)
        T = int(np.asarray(self.coords.t).size)
        if isinstance(groups, str):
            if groups != "band":
                raise ValueError(f'groups {groups!r}: "band", None or an integer array')
            groups = np.asarray(self.dets.band_index, np.int32)
        elif groups is not None:
            groups = np.asarray(groups)
            if groups.ndim != 1 or groups.dtype.kind not in "iu" or (groups.size and groups.min() < -1):
                raise ValueError("groups must be a one-dimensional integer array with entries >= -1")
            groups = groups.astype(np.int32)
        G = 1 if groups is None or not groups.size else max(int(groups.max()) + 1, 1)
        _tod_args.check_count(G, "the number of groups", regress.MAX_GROUPS)
        if int(poly_order) != poly_order or int(poly_order) < 0 or 2 + int(poly_order) + bool(airmass) > regress.MAX_TEMPLATES:
            raise ValueError(f"poly_order {poly_order}: an integer >= 0 with 2 + poly_order + airmass <= {regress.MAX_TEMPLATES}")
        extra = [regress.legendre_templates(T, int(poly_order))[1:]]
        if airmass:
            extra.append(regress.airmass_template(self.coords._bel)[None])
        extra = np.concatenate(extra)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        c, a, gains, ok, B = regress.fit_common_mode(signal, groups=groups, n_groups=G, flags=flags, model=model,
                                                     extra=extra if extra.shape[0] else None, n_iter=n_iter, min_hits=min_hits,
                                                     rcond=rcond, ctx=ctx)
        del signal
        regress.apply(data[into], B, a, groups=groups, sign=-1, out=data[into], ctx=ctx)
        metadata = dict(self.metadata)
        a_host = a.cpu().numpy()
        grouped = np.ones(a_host.shape[0], bool) if groups is None else groups >= 0  # a detector left out has not failed
        metadata["common_mode"] = {"n_groups": G, "n_iter": int(n_iter), "poly_order": int(poly_order), "airmass": bool(airmass),
                                   "min_hits": min_hits, "rcond": float(rcond), "gains": gains.cpu().numpy(), "offsets": a_host[:, 0].copy(),
                                   "coefficients": a_host, "common_mode": c.cpu().numpy(), "failed_rows": np.flatnonzero(~ok.cpu().numpy() & grouped)}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=self.flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def filter_subscans(self, order=3, bounds=None, turn_frac=0.9, flag_turnarounds=True, flag_failed=True, model=None, into=None,
                        min_hits=8, rcond=1e-10, ctx=None, device="cuda:0"):
        """A new TOD with a Legendre polynomial of degree ``order`` (0 .. 7) fitted to every detector's signal (the sum of
        the fields, less ``model``) in every subscan and subtracted from the field ``into`` (default: the first; the
        mappers bin the sum) (maria_amd.subscans).  The subscans are the stretches of the boresight azimuth
        between two turnarounds (``subscans.find_subscans`` with ``turn_frac``), or the segments of ``bounds`` [S + 1],
        ascending.  Samples with nonzero ``flags`` and the turnaround samples take no part in the fit, and are
        subtracted from like the rest of their segment.  A (detector, segment) pair with fewer than max(min_hits,
        order + 1) samples left, or whose polynomials are degenerate on them (``regress.solve``), is left bit for bit as
        it was.  The result's flags are the old ones, ORed with the turnarounds (``flag_turnarounds``) and with every
        sample of a segment that was not fitted (``flag_failed``).  Every field of the result is a float32 device copy;
        ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried over; ``metadata["subscans"]`` records
        ``order``, ``bounds``, ``turn_frac``, ``min_hits``, ``rcond``, the [D, S, order + 1] float64 ``coefficients`` and
        ``failed_segments``, the [n, 2] (detector, segment) pairs of the segments with samples that were not fitted.  This
        TOD is left as it is."""
        import torch

        from . import subscans

        if int(order) != order or not 0 <= int(order) < subscans.MAX_ORDER:
            raise ValueError(f"order {order}: an integer in 0 .. {subscans.MAX_ORDER - 1}")
        K = int(order) + 1
        min_hits = _tod_args.check_min_hits(min_hits)
        if not 0.0 <= float(rcond) < 1.0:
            raise ValueError(f"rcond {rcond}: in [0, 1)")
        T = int(np.asarray(self.coords.t).size)
        found, turn = subscans.find_subscans(self.coords._baz, turn_frac)
        if bounds is None:
            bounds = found
        else:
            bounds = np.asarray(bounds)
            if bounds.ndim != 1 or bounds.size < 2 or bounds.dtype.kind not in "iu" or np.any(np.diff(bounds.astype(np.int64)) < 0):
                raise ValueError("bounds must be a one-dimensional array of S + 1 >= 2 ascending integers")
            bounds = np.clip(bounds.astype(np.int64), 0, T).astype(np.int32)
        if turn.size != T:
            raise ValueError(f"the boresight has {turn.size} samples: the coordinates' time axis {T}")
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        dev = signal.device
        d_turn = torch.as_tensor(turn).to(dev)
        used = d_turn[None, :].expand(signal.shape[0], T).contiguous() if flags is None else flags | d_turn[None, :]
        d_bounds = torch.as_tensor(bounds).to(dev)
        a, ok = subscans.fit(signal, d_bounds, K, flags=used, model=model, min_hits=min_hits, rcond=rcond, ctx=ctx)
        del signal
        subscans.apply(data[into], d_bounds, a, sign=-1, out=data[into], ctx=ctx)
        segment = np.full(T, -1, np.int64)  # every sample's segment
        for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            segment[lo:hi] = s
        covered = torch.as_tensor(segment >= 0).to(dev)
        failed = ~ok[:, torch.as_tensor(np.maximum(segment, 0)).to(dev)] & covered[None, :]  # [D, T]
        new_flags = flags
        if flag_turnarounds:
            new_flags = used
        if flag_failed:
            new_flags = failed.to(torch.uint8) if new_flags is None else new_flags | failed.to(torch.uint8)
        nonempty = np.diff(bounds.astype(np.int64)) > 0
        metadata = dict(self.metadata)
        metadata["subscans"] = {"order": int(order), "bounds": np.array(bounds, np.int32), "turn_frac": float(turn_frac), "min_hits": min_hits,
                                "rcond": float(rcond), "coefficients": a.cpu().numpy(),
                                "failed_segments": np.argwhere(~ok.cpu().numpy() & nonempty[None, :])}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=new_flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def deconvolve_time_constants(self, tau=None, init="steady", into=None, ctx=None, device="cuda:0"):
        """A new TOD with the detectors' one-pole lag taken out of every field by its exact inverse, the two-tap FIR
        x[t] = (y[t] - a y[t - 1]) / (1 - a) with a = exp(-1 / (fs tau)) (maria_amd.time_constants).  It is
        the first step of time-domain cleaning, before anything is flagged or fitted: deconvolve_time_constants ->
        downsample -> flag_glitches -> fix_jumps -> remove_ground -> remove_common_mode -> filter_subscans -> cut.  A pipeline
        sees only the sum of the fields and the operation is linear, so every field is deconvolved, the noise with
        them (the FIR raises white noise towards the Nyquist frequency by up to (1 + a) / (1 - a); ``downsample`` is the
        next step and low-passes).  ``tau``: seconds, a scalar or one per detector (None: ``dets.time_constant``); an
        explicit value lets one study a mis-estimated time constant.  ``init``: "steady" (the detector had seen the first
        sample for ever, what ``Simulation`` applies) or "zero".  ``into``: accepted like the other steps' (a field's
        name); every field is treated alike.  fs is (n - 1) / (t[-1] - t[0]) as in ``psd``.  Flags: sample t of the
        result is flagged if t or t - 1 was, for its value depends on both.  On a TOD that was downsampled it raises
        NotImplementedError: at the reduced rate the lag is no longer one pole, so deconvolve first.  Every field of the
        result is a float32 device copy; ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried over
        (the conversion scales a row by a factor that changes over many time constants; exact where the run was made in
        pW); ``metadata["time_constants"]`` gains ``deconvolved`` True, ``deconvolved_tau`` and ``deconvolved_init``.  This TOD
        is left as it is."""
        import torch

        from . import time_constants

        if "downsample" in self.metadata:
            raise NotImplementedError("deconvolve_time_constants on a downsampled TOD: at the reduced rate the lag is no longer one "
                                      "pole; deconvolve first, then downsample")
        time_constants._check_init(init)
        n = int(self.dets.n)
        tau = np.asarray(self.dets.time_constant if tau is None else tau, float)
        if tau.ndim > 1 or (tau.ndim == 1 and tau.shape[0] != n):
            raise ValueError(f"tau must be a scalar or one time constant for each of the {n} detectors")
        a = time_constants.poles(np.broadcast_to(tau, (n,)), time_constants.sample_rate_of(self.coords.t))
        data, signal, _, flags, into, ctx = self._device_fields(None, into, ctx, device)
        d_a = torch.as_tensor(a).to(signal.device)
        del signal
        for x in data.values():
            time_constants.deconvolve(x, d_a, init=init, out=x, ctx=ctx)
        if flags is not None:
            grown = flags.clone()
            grown[:, 1:] |= flags[:, :-1]
            flags = grown
        metadata = dict(self.metadata)
        metadata["time_constants"] = dict(metadata.get("time_constants") or {}, deconvolved=True, deconvolved_tau=np.broadcast_to(tau, (n,)).copy(),
                                          deconvolved_init=init)
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def _segment_bounds(self, bounds):
        """[S + 1] int32 bounds for ``stats`` and ``cut``, clamped to 0 .. T: None (the whole row), "subscans"
        (``subscans.find_subscans`` of the boresight azimuth), an int (chunks of that many samples) or an ascending
        integer array."""
        from . import cuts, subscans

        T = int(np.asarray(self.coords.t).size)
        if bounds is None:
            return np.array([0, T], np.int32)
        if isinstance(bounds, str):
            if bounds != "subscans":
                raise ValueError(f'bounds {bounds!r}: None, "subscans", a chunk length or an integer array')
            found, _ = subscans.find_subscans(self.coords._baz)
            if found[-1] != T:
                raise ValueError(f"the boresight has {found[-1]} samples: the coordinates' time axis {T}")
            return found
        if isinstance(bounds, (int, np.integer)) and not isinstance(bounds, bool):
            return cuts.chunk_bounds(T, bounds)
        bounds = np.asarray(bounds)
        if bounds.ndim != 1 or bounds.size < 2 or bounds.dtype.kind not in "iu" or np.any(np.diff(bounds.astype(np.int64)) < 0):
            raise ValueError("bounds must be a one-dimensional array of S + 1 >= 2 ascending integers")
        return np.clip(bounds.astype(np.int64), 0, T).astype(np.int32)

    def stats(self, bounds=None, model=None, ctx=None, device="cuda:0"):
        """The statistics of the signal (the sum of the fields, less ``model``) over the samples whose ``flags`` are 0
        (maria_amd.cuts): a dict of ``bounds`` (the [S + 1] int32 segments used), ``segments`` (the
        summary of ``cuts.summarize`` per (detector, segment): [D, S] float64 device tensors ``mean``, ``var``, ``std``,
        ``skew``, ``kurtosis``, ``min``, ``max``, ``ptp``, ``sigma_diff``, ``flagged_fraction``, and int64 ``hits`` and
        ``pairs``) and ``detectors`` (the same per detector, [D], from a second pass with the row as one segment).
        ``bounds``: None (the whole row), "subscans" (``subscans.find_subscans``), an int (chunks of that many
        samples) or an ascending integer array.  This TOD is left as it is."""
        bounds = self._segment_bounds(bounds)
        _, signal, model, flags, _, ctx = self._device_fields(model, None, ctx, device)
        from . import cuts

        seg = cuts.summarize(cuts.moments(signal, bounds, flags=flags, model=model, ctx=ctx), np.diff(bounds.astype(np.int64)))
        det = seg if len(bounds) == 2 else cuts.summarize(cuts.moments(signal, None, flags=flags, model=model, ctx=ctx), [signal.shape[1]])
        return {"bounds": bounds, "segments": seg, "detectors": {k: v[:, 0] for k, v in det.items()}}

    def cut(self, bounds="subscans", groups="band", n_sigma=5.0, n_sigma_segment=5.0, max_flagged=0.5, max_bad_segments=0.5, min_hits=8,
            criteria=("white", "rms", "skew", "kurtosis", "flagged"), value=1, model=None, ctx=None, device="cuda:0"):
        """A new TOD whose flags also cover the detectors and the segments that are not worth mapping (maria_amd.cuts,
        DESIGN 3.26); the last step of time-domain cleaning, after ``filter_subscans``.  The statistics of :meth:`stats`
        are taken on the signal (the sum of the fields, less ``model``) over the samples whose flags are 0, per detector
        and per segment of ``bounds`` (as in :meth:`stats`).  A detector is cut whole if, within its group (``groups``:
        "band", None for one group, or an integer array, -1 leaving a detector out), it lies more than ``n_sigma``
        robust scales (1.4826 times the median absolute deviation) from the median in log ``sigma_diff`` ("white"),
        log ``std`` ("rms"), ``skew`` or ``kurtosis``, if more than ``max_flagged`` of its samples are flagged
        ("flagged"), or if it is unusable: fewer than max(min_hits, 1) samples kept, or one of those values not finite
        (a constant row).  A segment is bad if its ``sigma_diff`` lies more than ``n_sigma_segment`` robust scales
        above the median over that detector's own segments (``cuts.bad_segments``; None: segments are not judged); a
        detector with more than ``max_bad_segments`` of its non-empty segments bad is cut whole.  The segments are
        judged first and the detectors on what is left, the bad segments flagged: one noisy subscan does not cost the
        detector.  ``criteria`` picks among the five names.
        ``value`` (1 .. 255) is ORed into the flags of every sample of a cut detector and of a bad segment
        (``cuts.flag_segments``); the mappers give flagged samples no weight.  Every field of the result is a float32
        device copy, unchanged; ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried over;
        ``metadata["cuts"]`` records the parameters, ``bounds``, the per-criterion [D] bool ``masks`` (with "unusable"
        and "segments"), ``cut_detectors`` (indices), ``cut_segments`` (the [n, 2] (detector, segment) pairs flagged in
        detectors that were not cut whole) and ``flagged_fraction_before`` / ``flagged_fraction_after``.  This TOD is
        left as it is."""
        import torch

        from . import cuts

        bounds = self._segment_bounds(bounds)
        if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= 255:
            raise ValueError(f"value {value}: an integer in 1 .. 255")
        if isinstance(groups, str):
            if groups != "band":
                raise ValueError(f'groups {groups!r}: "band", None or an integer array')
            groups = np.asarray(self.dets.band_index, np.int64)
        elif groups is not None:
            groups = np.asarray(groups)
            if groups.ndim != 1 or groups.dtype.kind not in "iu" or (groups.size and groups.min() < -1):
                raise ValueError("groups must be a one-dimensional integer array with entries >= -1")
            groups = groups.astype(np.int64)
        cuts._check_rules(n_sigma, n_sigma_segment, max_flagged, max_bad_segments, min_hits, criteria)
        data, signal, model, flags, _, ctx = self._device_fields(model, None, ctx, device)
        D, T = signal.shape
        if groups is not None and groups.shape[0] != D:
            raise ValueError(f"groups must have one entry for each of the {D} detectors")
        seg = cuts.summarize(cuts.moments(signal, bounds, flags=flags, model=model, ctx=ctx), np.diff(bounds.astype(np.int64)))
        bad = cuts.bad_segments(seg, groups, n_sigma_segment, min_hits)
        new_flags = torch.zeros((D, T), dtype=torch.uint8, device=signal.device) if flags is None else flags.clone()
        before = float((new_flags != 0).sum()) / new_flags.numel()
        if bool(bad.any()):
            cuts.flag_segments(new_flags, bounds, bad, value=int(value), ctx=ctx)
        det = cuts.summarize(cuts.moments(signal, None, flags=new_flags, model=model, ctx=ctx), [T])  # without the bad segments
        del signal
        masks, cut = cuts.decide(det, seg, bad, groups, n_sigma, max_flagged, max_bad_segments, min_hits, criteria)
        if bool(cut.any()):
            cuts.flag_segments(new_flags, np.array([0, T], np.int32), cut[:, None], value=int(value), ctx=ctx)
        metadata = dict(self.metadata)
        metadata["cuts"] = {"bounds": np.array(bounds, np.int32), "n_sigma": float(n_sigma),
                            "n_sigma_segment": None if n_sigma_segment is None else float(n_sigma_segment), "max_flagged": float(max_flagged),
                            "max_bad_segments": float(max_bad_segments), "min_hits": int(min_hits), "criteria": tuple(criteria), "value": int(value),
                            "groups": None if groups is None else groups.copy(), "masks": {k: v.cpu().numpy() for k, v in masks.items()},
                            "cut_detectors": np.flatnonzero(cut.cpu().numpy()), "cut_segments": np.argwhere((bad & ~cut[:, None]).cpu().numpy()),
                            "flagged_fraction_before": before, "flagged_fraction_after": float((new_flags != 0).sum()) / new_flags.numel()}
        out = TOD(data=data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=new_flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def with_offsets(self, offsets):
        """A TOD that shares this one's data, flags and metadata and whose ``coords.offsets`` and ``dets.offsets`` are
        ``offsets`` [D, 2] (radians): a fitted table (``BeamFit.offsets()``) on its way into any mapper, or the nominal
        table in place of the true one."""
        offsets = np.array(offsets, float)
        if offsets.shape != (self.dets.n, 2) or not np.all(np.isfinite(offsets)):
            raise ValueError(f"offsets must be [{self.dets.n}, 2] finite numbers (radians)")
        import copy

        dets = copy.copy(self.dets)
        dets.offsets = offsets
        out = TOD(data=self.data, dets=dets, coords=self.coords.broadcast(offsets), units=self.units, metadata=self.metadata, flags=self.flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def beam_fwhm(self):
        """[D] radians: the detector table's own beam FWHM, the one the simulation smooths a map with
        (``compute_angular_fwhm`` of the mean ``primary_size`` at the detector's band centre)."""
        from .instrument import compute_angular_fwhm

        return np.asarray(compute_angular_fwhm(fwhm_0=float(self.dets.primary_size.mean()), z=np.inf, nu=self.dets.band_center), float)

    def _source_frame(self, source, frame, src_track, degrees, device):
        """(pointing dict of device tensors, centre (phi, theta) in radians, src [T, 2] or None) for ``mask_source`` and
        ``fit_beams``: the frame's transform, the boresight and the detector table as the mappers hand them to the binning.
        ``source`` None: the scan centre, the mean direction of the boresight in the frame."""
        import torch

        if frame not in ("ra/dec", "az/el"):
            raise NotImplementedError(f"frame '{frame}': only 'ra/dec' and 'az/el' are built")
        unit = np.pi / 180 if degrees else 1.0
        T = int(np.asarray(self.coords.t).size)
        stack = sky_transform_stack(self.coords.t, self.metadata["latitude"], self.metadata["longitude"]) if frame == "ra/dec" else None
        if source is None:
            from .beamfit import scan_center

            center = scan_center(self.coords._baz, self.coords._bel, stack)
        else:
            source = np.asarray(source, float)
            if source.shape != (2,) or not np.all(np.isfinite(source)):
                raise ValueError("source must be (phi, theta): two finite angles")
            center = (float(unit * source[0]), float(unit * source[1]))
        if src_track is not None:
            src_track = unit * np.asarray(src_track, float)
            if src_track.shape != (T, 2) or not np.all(np.isfinite(src_track)):
                raise ValueError(f"src_track must be [{T}, 2] finite offsets from the source's nominal position")
            src_track = torch.as_tensor(np.ascontiguousarray(src_track, np.float32)).to(device)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
        point = {"az": f32(self.coords._baz), "el": f32(self.coords._bel),
                 "transform": None if stack is None else torch.as_tensor(stack.reshape(-1, 9)).to(device),
                 "dx": f32(self.coords.offsets[:, 0]), "dy": f32(self.coords.offsets[:, 1])}
        return point, center, src_track

    def mask_source(self, source=None, radius=None, frame="ra/dec", src_track=None, value=1, degrees=True, ctx=None, device="cuda:0"):
        """A TOD whose flags also cover the neighbourhood of a point source (maria_amd.beamfit.source_flags):
        ``value`` (1 .. 255) is ORed into the flags of every sample at which the detector, at its table offset, points
        within ``radius`` of the source; the flags are created if the TOD has none.  ``source``: (phi, theta) in
        ``frame`` ("ra/dec" or "az/el"), None for the scan centre; ``radius``: None for 3 x the largest beam FWHM of the
        detector table; ``src_track`` [T, 2]: the source's offsets from ``source`` at every sample (a planet that
        moves); angles in degrees with ``degrees``, else radians.  ``remove_common_mode`` and ``filter_subscans`` leave
        flagged samples out of their fits, so a bright source masked first does not bias them.  The data are shared with
        this TOD, which is left as it is."""
        import torch

        from . import beamfit

        if radius is None:
            radius = 3.0 * float(self.beam_fwhm().max())
        else:
            radius = float(radius) * (np.pi / 180 if degrees else 1.0)
        if not (np.isfinite(radius) and radius >= 0):
            raise ValueError(f"radius {radius}: finite and >= 0")
        dev = torch.device(device) if self.flags is None or not torch.as_tensor(self.flags).is_cuda else torch.as_tensor(self.flags).device
        point, center, src = self._source_frame(source, frame, src_track, degrees, dev)
        D, T = int(self.dets.n), int(np.asarray(self.coords.t).size)
        flags = torch.zeros((D, T), dtype=torch.uint8, device=dev) if self.flags is None else torch.as_tensor(self.flags).to(dev, torch.uint8).clone()
        beamfit.source_flags(point, center, radius, src=src, inside=True, value=value, flags=flags, ctx=ctx)
        metadata = dict(self.metadata)
        metadata["source_mask"] = {"center": center, "radius": radius, "frame": frame, "value": int(value)}
        out = TOD(data=self.data, dets=self.dets, coords=self.coords, units=self.units, metadata=metadata, flags=flags)
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def fit_beams(self, source=None, frame="ra/dec", radius=None, elliptical=False, field=None, model=None, src_track=None, n_iter=20,
                  degrees=True, ctx=None, device="cuda:0"):
        """``beamfit.BeamFit``: every detector's beam, pointing offset and gain from this scan over a point source
        (maria_amd.beamfit).  The signal is the sum of the fields (or the one ``field``), less ``model``.
        The window is ``radius`` (None: 3 x the detector's own beam FWHM of the table, per band the largest) around the
        source at the NOMINAL offsets of the table, ANDed with ``flags == 0``; it is fixed once.  The starting point
        comes from ``cuts.moments`` over the window: c0 = mean, A0 = max - mean, the width from the detector table, the
        offsets the nominal ones.  ``source``, ``frame``, ``src_track``, ``degrees`` as in :meth:`mask_source`.  Run
        it on a source scan after ``flag_glitches`` / ``fix_jumps`` and before anything that filters (or filter with
        the source masked); ``with_offsets(fit.offsets())`` then goes into any mapper, and ``fit.relative_gain()`` is
        the flat field.  This TOD is left as it is."""
        import torch

        from . import beamfit, cuts

        if field is not None and field not in self.data:
            raise ValueError(f"field {field!r}: one of the fields {self.fields}")
        fwhm = self.beam_fwhm()
        if radius is None:
            radius = 3.0 * float(fwhm.max())
        else:
            radius = float(radius) * (np.pi / 180 if degrees else 1.0)
        if not (np.isfinite(radius) and radius > 0):
            raise ValueError(f"radius {radius}: finite and > 0")
        _, signal, model, flags, _, ctx = self._device_fields(model, None, ctx, device)
        if field is not None:
            v = self.data[field]
            signal = (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(signal.device, torch.float32).contiguous()
        D, T = signal.shape
        point, center, src = self._source_frame(source, frame, src_track, degrees, signal.device)
        window = torch.zeros((D, T), dtype=torch.uint8, device=signal.device) if flags is None else (flags != 0).to(torch.uint8)
        beamfit.source_flags(point, center, radius, src=src, inside=False, value=1, flags=window, ctx=ctx)
        m = cuts.moments(signal, None, flags=window, model=model, ctx=ctx)
        mean, peak = m.mean[:, 0], m.max[:, 0]
        w0 = torch.as_tensor((beamfit.FWHM_PER_SIGMA / fwhm) ** 2).to(signal.device)
        init = torch.stack([peak - mean, point["dx"].to(torch.float64), point["dy"].to(torch.float64), w0, mean], dim=1)
        return beamfit.fit(signal, point, center, init, window, model=model, src=src, elliptical=elliptical, n_iter=n_iter,
                           groups=np.asarray(self.dets.band_index, np.int64), ctx=ctx)

    def to(self, units):
        """tod/tod.py:106-142 between "pW" and "K_RJ" (``mrx_tod_to_krj`` / ``mrx_tod_from_krj`` on
        every field), for a TOD that came out of ``Simulation.run``; other units stay with maria's
        calibration graph."""
        if units == self.units:
            return self
        if {units, self.units} != {"pW", "K_RJ"} or getattr(self, "_calibrator", None) is None:
            raise NotImplementedError(
                f"conversion {self.units} -> {units}: only pW <-> K_RJ of a TOD made by Simulation.run() is built"
            )
        out = TOD(data=self._calibrator(self.data, to_krj=(units == "K_RJ")), dets=self.dets, coords=self.coords, units=units,
                  metadata=self.metadata, flags=self.flags)
        out._calibrator = self._calibrator
        return out


class Simulation:
    def __init__(
        self,
        instrument,
        plans,
        site,
        atmosphere=None,
        atmosphere_kwargs: dict = {},
        cmb=None,
        cmb_kwargs: dict = {},
        map=None,
        map_kwargs: dict = {},
        noise: bool = True,
        noise_kwargs: dict = {},
        progress_bars: bool = True,
        keep_mean_signal: bool = False,
        dtype: type = np.float32,
        *,
        gain_seed: int = None,
        noise_seed: int = None,
        device_output: bool = False,
        shard=None,
        device: str = "cuda:0",
        hwp=None,
    ):
        """sim/simulation.py:76-198.  ``device_output=True`` leaves the TOD on the GPU as
        a torch tensor (a 10 k x 240 k TOD is 9.6 GB; the PCIe copy dwarfs the synthesis).
        ``shard``: ``(rank, world_size)`` -- this process simulates its contiguous block of
        detector rows (maria_amd.dist.shard_slice) of every observation, ``"auto"`` takes both
        from an initialised ``torch.distributed`` group, ``None`` simulates every row.  Every
        detector row is independent given the shared geometry (atmosphere.py:346-373 has no
        cross-detector term), so a shard's TOD equals the same rows of the unsharded run.
        ``hwp``: a maria_amd.hwp.HWP, a continuously rotating ideal half-wave plate in front of the detectors: the
        ``map`` field becomes S_I + S_c cos 4 chi + S_s sin 4 chi (atmosphere and noise are not modulated),
        and ``TOD.demodulate`` takes it apart again.  None: no plate, and the bits of every run are what they were."""
        if hwp is not None:
            from .hwp import HWP

            if not isinstance(hwp, HWP):
                raise TypeError("'hwp' must be a maria_amd.hwp.HWP")
        self.hwp = hwp
        if cmb is not None:
            raise NotImplementedError("the CMB mixin is a follow-on row (SURVEY 8(f))")
        if isinstance(map, str):
            raise NotImplementedError("reading a map from a file stays with maria's io; pass a maria_amd.map.ProjectionMap")
        if map is not None:
            from .map import ProjectionMap

            if not isinstance(map, ProjectionMap):
                raise TypeError("'map' must be a maria_amd.map.ProjectionMap")
        self.map, self.map_kwargs = map, {"bilinear_sampling": True, **dict(map_kwargs)}  # sim/map.py:20
        if np.dtype(dtype) != np.float32:
            raise NotImplementedError("the device path writes float32 TODs (the reference default)")
        if not isinstance(instrument, Instrument):
            raise ValueError("'instrument' must be an Instrument (named configs stay with maria's front end)")
        if not isinstance(site, Site):
            raise ValueError("'site' must be either a Site object or a string.")
        if isinstance(plans, Plan):
            plans = [plans]
        elif not isinstance(plans, list):
            raise TypeError("plans must be a plan or a list of plans")
        self.instrument, self.site, self.plans = instrument, site, plans
        self.atmosphere, self.atmosphere_kwargs = atmosphere, dict(atmosphere_kwargs)
        self.noise, self.dtype = noise, dtype
        self.disable_progress_bars = not progress_bars
        self.device_output = device_output
        self.device = device  # every observation of this Simulation runs on this GPU
        if shard == "auto":
            import torch.distributed as dist

            shard = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else None
        if shard is not None:
            rank, world = (int(v) for v in shard)
            if not 0 <= rank < world:
                raise ValueError(f"shard rank {rank} outside [0, {world})")
            shard = (rank, world)
        self.shard = shard
        if shard is not None and shard[1] > 1:
            bands = instrument.dets.bands if isinstance(instrument, Instrument) else []
            if noise and noise_seed is None:
                raise ValueError("a sharded run needs an explicit noise_seed: the correlated noise modes are common to all shards")
            if gain_seed is None and any(getattr(b, "gain_error", 0.0) for b in bands):
                raise ValueError("a sharded run needs an explicit gain_seed: every rank draws the whole gain vector and keeps its rows")
        self._gain_rng = np.random.default_rng(gain_seed)
        self.noise_kwargs = dict(noise_kwargs)
        self._noise_seed = int(noise_seed if noise_seed is not None else np.random.SeedSequence().entropy % (1 << 62))
        self._noise_runs = 0
        self._noise_ctx = None
        self.obs_list = []
        for plan in self.plans:
            obs = Observation(instrument, plan, site, atmosphere, {"device": device, **self.atmosphere_kwargs})
            if hasattr(obs, "atmosphere"):
                # only the map mixin reads the coarse pwv (sim/map.py:117-135): without it the sampler and
                # the TOD writer run pipelined in one call and the pwv is made if somebody asks for it
                obs.atmosphere.keep_pwv = self.map is not None
                obs.atmosphere.initialize(obs)
            self.obs_list.append(obs)

    def _rows(self, n_det):
        """[lo, hi) of this process's detector rows (all of them without a shard)."""
        if self.shard is None:
            return 0, n_det
        from .dist import shard_bounds

        return shard_bounds(n_det, self.shard[1], self.shard[0])

    def run(self, units: str = "K_RJ", gather: bool = False):
        """sim/simulation.py:201-211: one TOD per plan, in ``units`` ("K_RJ", the reference
        default, or "pW").  With a shard each TOD holds this rank's rows; ``gather=True``
        all-gathers every field over the initialised ``torch.distributed`` group (RCCL over
        xGMI for device tensors) into the whole [ndet, nt] arrays on every rank."""
        if units not in ("K_RJ", "pW"):
            raise NotImplementedError(f"units '{units}': only 'K_RJ' and 'pW' are built (tod/tod.py:106-142)")
        tods = []
        for k, obs in enumerate(self.obs_list):
            t0 = ttime.monotonic()
            tod = self.run_obs(obs, units=units)
            if gather and self.shard is not None and self.shard[1] > 1:
                tod = self._gather(obs, tod)
            tods.append(tod)
            logger.info(f"Simulated observation {k + 1} of {len(self.obs_list)} in {ttime.monotonic() - t0:.2f} s")
        return tods

    # -- sim/atmosphere.py:24-84 -------------------------------------------------------
    def _simulate_atmosphere(self, obs):
        lo, hi = self._rows(obs.instrument.dets.n)
        det_slice = None if self.shard is None else slice(lo, hi)
        # screens only: DevicePath.run() samples and writes in one call -- with a map too: the coarse pwv its calibration
        # reads (sim/map.py:117-135) is the sampler's second output there (keep_pwv)
        obs.atmosphere.new_realisation(instrument=obs.instrument, det_slice=det_slice)

    def _gather(self, obs, tod):
        """All-gather a shard's TOD along the detector axis (equal row blocks, so the gathered
        array is the concatenation: dist.all_gather_tod)."""
        import torch

        from .dist import all_gather_tod

        dets = obs.instrument.dets
        data = {}
        for name, field in tod.data.items():
            on_device = isinstance(field, torch.Tensor)
            full = all_gather_tod(field if on_device else torch.as_tensor(field), dets.n)
            data[name] = full if on_device else full.numpy()
        out = TOD(data=data, dets=dets, coords=obs.coords, units=tod.units, metadata=dict(tod.metadata, shard=None))
        return out

    def _set_calibration(self, obs, metadata):
        """Host part of ``TOD.to("K_RJ")`` (tod/tod.py:90-97): collapse the bands' transmission
        tables at the scalars the TOD metadata carries, rounded as run_obs stores them."""
        atm, dets = obs.atmosphere, obs.instrument.dets
        path = atm._device_path()
        key = (metadata["base_temperature"], metadata["pwv"])
        # (the key lives on the path itself: a path rebuilt for another shard has none, whatever address it got)
        if path._cal_key == key and path._cal is not None:  # same path, same scalars: the tables are on the device already
            return
        path._cal_key = key
        sp = atm.spectrum
        tables = [{"T": sp.side_base_temperature, "pwv": sp.side_zenith_pwv, "el": sp.side_elevation,
                   "values": band.transmission_table(sp)} for band in dets.bands]
        polarized = [bool((~np.isnan(dets.gamma[dets.band_index == b])).all()) for b in range(len(dets.bands))]
        atm._device_path().set_calibration(tables, metadata["base_temperature"], metadata["pwv"], obs.boresight.el,
                                           obs.coords.offsets, polarized)

    def _compute_atmospheric_loading(self, obs, gain=None, units="pW", metadata=None):
        """Spline solve + cubic upsample of the coarse loading the sampling kernel already
        wrote (emission and Mueller weight are fused into it), scaled by ``gain``; with
        ``units="K_RJ"`` the division of ``TOD.to`` (tod/tod.py:90-142) is fused in: on the coarse grid
        before the spline where ``DevicePath.coarse_krj_bound`` allows, per sample in the writer otherwise."""
        import torch

        path = obs.atmosphere._device_path()
        path.set_gain(gain)
        out = torch.empty((path.D, path.T), dtype=torch.float32, device=path.device)
        if units == "K_RJ":
            self._set_calibration(obs, metadata)
        path.run(out, krj=units == "K_RJ")  # (nothing is sampled yet: see _simulate_atmosphere)
        path.check_flags()  # RuntimeError "introduced nans" like atmosphere.py:368-369
        return out

    def _sample_maps(self, obs, rows=None, krj=None, gain=None, stokes_rows=None):
        """sim/map.py:76-172 on the device: one ``mrx_map_sample`` per band, [D, T] pW
        (``rows = (lo, hi)``: only this shard's detector rows).  ``krj`` (``DevicePath.krj_row_tables()``): the field in
        K_RJ instead, ``gain`` [D] multiplied in, both on the sampler's own store (``mrx_map_sample_krj``: the bits of
        the pW field times the gain, converted by ``DevicePath.to_krj``, without the two passes over the field).
        ``stokes_rows``: [rows, 4] (I, Q, U, V) weights of this call in place of the detectors' cached Mueller rows."""
        import torch

        from . import map as mmap
        from ._lib import Context
        from .instrument import compute_angular_fwhm

        lo, hi = rows or (0, obs.instrument.dets.n)
        dets = obs.instrument.dets.subset(np.arange(lo, hi))
        offsets = obs.coords.offsets[lo:hi]
        atm = getattr(obs, "atmosphere", None)
        if atm is not None:
            path = atm._device_path()
            ctx, device = path.ctx, path.device
            # (sync=False below frees this call's temporaries while the kernel is in flight: safe only on torch's current
            # stream, whatever stream path.run() left on the context)
            ctx.set_stream(torch.cuda.current_stream(device))
        else:
            device = torch.device(self.device)
            self._noise_ctx = self._noise_ctx or Context(device.index or 0)
            ctx = self._noise_ctx
            ctx.set_stream(torch.cuda.current_stream(device))
        T = len(obs.coords.t)
        # what does not change from run to run lives on the device, per observation and per band: the boresight, the
        # sample times, the horizon -> equatorial transform (14 ms of host arithmetic and 17 MB a run when it was made
        # per call), the smoothed map channels, the collapsed calibration tables, the detectors' offsets and weights
        # (the map OBJECT is kept and compared with `is`, as are the things the cached tensors were made from -- its data
        # array and the weather's temperature: an id() of a freed map can come back, and an edit in place keeps the id)
        key = (str(device), lo, hi)
        made_from = (self.map, self.map.data, None if atm is None else float(atm.weather.temperature[0]))
        cache = getattr(obs, "_map_cache", None)
        if (cache is None or cache.get("key") != key or cache["made_from"][0] is not made_from[0]
                or cache["made_from"][1] is not made_from[1] or cache["made_from"][2] != made_from[2]):
            f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
            f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64)).to(device)  # noqa: E731
            cache = {"key": key, "made_from": made_from, "az": f32(obs.boresight._baz), "el": f32(obs.boresight._bel),
                     "t": f64(obs.coords.t), "bands": {}}
            if atm is not None:
                cache["steps_per_tile"] = mmap.steps_per_tile(obs.coords.t, atm._device_path().dta)
            cache["transform"] = (f64(sky_transform_stack(obs.coords.t, obs.site.latitude, obs.site.longitude).reshape(T, 9))
                                  if self.map.frame == "ra/dec" else None)
            mueller_rows = mmap.mueller_row(dets.gamma)[:, ["IQUV".index(s) for s in self.map.stokes]]
            covered = np.zeros(dets.n, bool)
            for b, band in enumerate(dets.bands):
                idx = np.nonzero(dets.band_index == b)[0]
                if len(idx) == 0:
                    continue
                # ideally one beam per channel; the reference smooths once per band (map.py:101-104)
                fwhm = float(compute_angular_fwhm(fwhm_0=dets.primary_size.mean(), z=np.inf, nu=band.center))
                smoothed = self.map.smooth(fwhm, ctx=ctx, device=device)  # [S, C, eta, xi]
                channels, tables, scalars = [], [], []
                for c, (nu_min, nu_max) in enumerate(self.map.nu_bin_bounds):
                    if band.nu.max() < nu_min or nu_max < band.nu.min():  # map.py:112-113
                        continue
                    channels.append(c)
                    if atm is not None:  # band/band.py:250-255
                        sp = atm.spectrum
                        mask = (sp.side_nu >= nu_min) & (sp.side_nu < nu_max)
                        nu = sp.side_nu[mask]
                        grid = np.trapezoid(band.passband(nu) * np.exp(-sp._opacity[..., mask]), x=nu, axis=-1)
                        tables.append(mmap.collapse_temperature(grid, sp.side_base_temperature, atm.weather.temperature[0]))
                    else:  # band/band.py:246-248
                        nu = band.nu[(band.nu >= nu_min) & (band.nu < nu_max)]
                        scalars.append(float(np.trapezoid(band.passband(nu), x=nu)))
                if not channels:
                    logger.warning(f"No load from map for band {band.name}")
                    continue
                covered[idx] = True
                sm = smoothed if isinstance(smoothed, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(smoothed, np.float32))
                entry = dict(idx=idx, contiguous=bool((np.diff(idx) == 1).all()),
                             values=sm.to(device, torch.float32)[:, channels].transpose(0, 1).contiguous(),  # [C, S, eta, xi]
                             offsets=f32(offsets[idx]), stokes=f64(mueller_rows[idx]), idx_dev=torch.as_tensor(idx, device=device))
                if atm is not None:
                    sp = atm.spectrum
                    entry.update(tab=f32(np.stack(tables)), ap=f32(sp.side_zenith_pwv), ae=f32(sp.side_elevation))
                else:
                    entry.update(scalars=scalars)
                cache["bands"][b] = entry
            cache["all_rows"] = bool(covered.all())
            obs._map_cache = cache
        # rows of bands that see no channel of the map stay zero (sim/map.py:112-113); where every row is written
        # nothing is cleared first (a [D, T] fill is 9.6 GB at the headline size)
        out = (torch.empty if cache["all_rows"] else torch.zeros)((dets.n, T), dtype=torch.float32, device=device)
        for b, e in cache["bands"].items():
            # the reference masks rows by band name (sim/map.py:90-95): a band's rows need not be neighbours.  Contiguous
            # rows are written in place; scattered ones into a buffer of their own, copied to their rows below
            idx = e["idx"]
            if atm is not None:
                pwv = path.coarse_pwv_time_major(e["idx_dev"])  # [Ta, D_band]
                kw = dict(cal_tables=e["tab"], cal_axis_pwv=e["ap"], cal_axis_el=e["ae"], coarse_pwv=pwv, ta0=path.ta0,
                          dta=path.dta, t=cache["t"], steps_per_tile=cache["steps_per_tile"])
            else:
                kw = dict(cal_scalars=e["scalars"])
            if krj is not None:  # the calibration's per-row arrays for this band's rows (kept while the tables are the same objects)
                if e.get("krj_of") is not krj["dx"]:
                    e["krj_rows"] = {k: krj[k].index_select(0, e["idx_dev"]) for k in ("dx", "dy", "band")}
                    e["krj_of"] = krj["dx"]
                kw.update(krj=dict(e["krj_rows"], bore_el=krj["bore_el"], axis=krj["axis"], values=krj["values"]),
                          scale=None if gain is None else gain.index_select(0, e["idx_dev"]))
            dst = out[int(idx[0]) : int(idx[-1]) + 1] if e["contiguous"] else torch.empty((len(idx), T), dtype=torch.float32, device=device)
            stokes = e["stokes"]
            if stokes_rows is not None:
                picked = np.asarray(stokes_rows, np.float64)[idx][:, ["IQUV".index(s) for s in self.map.stokes]]
                stokes = torch.as_tensor(np.ascontiguousarray(picked)).to(device)
            mmap.sample_map(ctx, e["values"], self.map.eta, self.map.xi, self.map.center, cache["az"], cache["el"],
                            e["offsets"], stokes, out=dst, transform=cache["transform"],
                            bilinear=bool(self.map_kwargs["bilinear_sampling"]), device=device, sync=False, **kw)
            if not e["contiguous"]:
                out.index_copy_(0, e["idx_dev"], dst)
        return out

    def _simulate_noise(self, obs, loading=None, rows=None, krj=None):
        """sim/noise.py:18-63 on the device, in pW; ``loading`` (pW, [D, T] on the device) only
        for bands whose NEP grows with the loading.  The gain error does not apply to the
        noise field (simulation.py:243-245).  ``krj``: DevicePath.krj_row_tables() -- the field in K_RJ."""
        import torch

        from . import noise as mnoise
        from ._lib import Context

        dets = obs.instrument.dets
        if hasattr(obs, "atmosphere"):
            ctx, device = obs.atmosphere._device_path().ctx, obs.atmosphere._device_path().device
        else:
            device = torch.device(self.device)
            if self._noise_ctx is None:
                self._noise_ctx = Context(device.index or 0)
            ctx = self._noise_ctx
            ctx.set_stream(torch.cuda.current_stream(device))
        t = obs.coords.t
        fs = 1.0 / np.mean(np.diff(t)) if len(t) > 1 else 1.0
        self._noise_runs += 1
        return mnoise.simulate_noise(ctx, dets, len(t), fs, self._noise_seed + 104729 * self._noise_runs,
                                     self.noise_kwargs, device=device, loading=loading,
                                     det_slice=None if rows is None else slice(*rows), krj=krj)

    def run_obs(self, obs, units: str = "pW") -> TOD:
        """sim/simulation.py:213-272 (followed by ``.to(units)`` of :206), for this process's
        detector rows."""
        import torch

        from . import _lib

        obs.loading = {}
        all_dets = obs.instrument.dets
        lo, hi = self._rows(all_dets.n)
        rows = None if self.shard is None else (lo, hi)
        dets = all_dets if rows is None else all_dets.subset(np.arange(lo, hi))
        # per-detector gain error (simulation.py:239-247): every rank draws the whole vector
        # and keeps its rows
        gain_error = np.array([b.gain_error for b in all_dets.bands], float)[all_dets.band_index]  # (not a loop over the detectors: 0.6 ms for 10 000, with the GPU idle)
        if any(b.gain_error for b in all_dets.bands):
            gain = np.exp(gain_error * self._gain_rng.standard_normal(all_dets.n))[lo:hi]
        else:  # no band has a gain error: nothing to draw (every rank decides alike, so the streams stay in step)
            gain = np.ones(hi - lo)
        has_gain = bool(np.any(gain_error[lo:hi]))
        metadata = {"atmosphere": False, "altitude": float(obs.site.altitude), "region": obs.site.region,
                    "latitude": obs.site.latitude, "longitude": obs.site.longitude,
                    "shard": None if rows is None else {"rank": self.shard[0], "world": self.shard[1], "rows": [lo, hi]}}
        if self.hwp is not None:
            metadata["hwp"] = self.hwp.to_metadata()
        has_atm = hasattr(obs, "atmosphere")
        device = torch.device(obs.atmosphere.device) if has_atm else torch.device(self.device)
        # Detector time constants: the detector lags optical power and calibration follows, so with any of
        # this process's rows lagged the run is made in pW, the optical fields go through mrx_tod_onepole on the device,
        # and the finished TOD through TOD.to(units).  Where every tau is 0 nothing below changes.
        tau = self._time_constants(dets)
        lagged = tau is not None
        units_out = units
        # A half-wave plate modulates optical power too: the same precedent, the map field made in pW
        modulated = self.hwp is not None and self.map is not None
        if lagged or modulated:
            units = "pW"
        if hi <= lo:
            # a rank past the last block of rows (dist.shard_bounds cuts blocks of 16: 144 detectors on 4 ranks are
            # 48 + 48 + 48 + 0): fields of no rows, and the random streams kept in step with the other ranks
            if has_atm:
                metadata.update(atmosphere=True, pwv=float(np.round(obs.atmosphere.weather.pwv, 3)),
                                base_temperature=float(np.round(obs.atmosphere.weather.temperature[0], 3)))
                obs.atmosphere._realisation += 1
            names = [n for n, on in (("atmosphere", has_atm), ("map", self.map is not None), ("noise", self.noise)) if on]
            empty = torch.empty((0, len(obs.coords.t)), dtype=torch.float32, device=device)
            obs.loading = {n: (empty.clone() if self.device_output else empty.cpu().numpy()) for n in names}
            tod = TOD(data=obs.loading, dets=dets, coords=obs.boresight.broadcast(obs.coords.offsets[lo:hi]), units=units, metadata=metadata)
            tod._calibrator = lambda data, to_krj: {k: (v.clone() if isinstance(v, torch.Tensor) else v.copy()) for k, v in data.items()}
            return tod
        # Bands whose NEP grows with the loading need the loadings in pW, WITHOUT the gain
        # error, before the noise is drawn (sim/noise.py:35-37 runs before simulation.py:239-247
        # multiplies the gain into the non-noise fields); gain and the K_RJ conversion are then
        # applied after the fact.  Otherwise both ride on the upsample's store.
        loading_nep = self.noise and any(getattr(b, "NEP_per_loading", 0.0) for b in dets.bands)
        loading = None
        if has_atm:
            metadata.update(atmosphere=True, pwv=float(np.round(obs.atmosphere.weather.pwv, 3)),
                            base_temperature=float(np.round(obs.atmosphere.weather.temperature[0], 3)))
            self._simulate_atmosphere(obs)
            loading = self._compute_atmospheric_loading(
                obs, gain=gain if has_gain and not loading_nep else None,
                units="pW" if loading_nep else units, metadata=metadata)
        # The map field: in pW, gain and TOD.to("K_RJ") applied below -- or, in the default units with an atmosphere to
        # calibrate by and no noise that wants the loadings in pW first, written in K_RJ with the gain by the sampler
        # itself (mrx_map_sample_krj; not with the literal pointing chain, which that entry refuses)
        map_loading, map_done = None, False
        if self.map is not None:
            if (units == "K_RJ" and has_atm and not loading_nep
                    and not obs.atmosphere._device_path().ctx.get_option(_lib.OPT_POINTING_CHAIN)):
                self._set_calibration(obs, metadata)
                d_gain_rows = torch.as_tensor(gain.astype(np.float32), device=device) if has_gain else None
                map_loading = self._sample_maps(obs, rows, krj=obs.atmosphere._device_path().krj_row_tables(), gain=d_gain_rows)
                map_done = True
            elif modulated:
                map_loading = self._sample_hwp(obs, rows, dets)  # pW
            else:
                map_loading = self._sample_maps(obs, rows)  # pW
        noise = None
        if self.noise:
            total = None
            if loading_nep:  # noise.py:35-37 sums every loading field, in pW
                fields = [f for f in (loading, map_loading) if f is not None]
                if fields:
                    total = fields[0] if len(fields) == 1 else fields[0] + fields[1]
                else:
                    total = torch.zeros((dets.n, len(obs.coords.t)), dtype=torch.float32, device=device)
            # in the default units the noise leaves its generator in K_RJ (mrx_noise_generate_krj)
            noise_krj = None
            if units == "K_RJ" and has_atm:
                self._set_calibration(obs, metadata)
                noise_krj = obs.atmosphere._device_path().krj_row_tables()
            noise = self._simulate_noise(obs, loading=total, rows=rows, krj=noise_krj)
        if has_gain:  # the gain error applies to every field but the noise (simulation.py:243-245)
            d_gain = torch.as_tensor(gain.astype(np.float32), device=device)[:, None]
            if map_loading is not None and not map_done:
                map_loading *= d_gain
            if loading is not None and loading_nep:
                loading *= d_gain
        if units == "K_RJ" and has_atm:
            # TOD.to("K_RJ") of the fields that were not written in K_RJ directly
            path = obs.atmosphere._device_path()
            if loading_nep:
                self._set_calibration(obs, metadata)
                path.to_krj(loading)
            if map_loading is not None and not map_done:  # (the noise was written in K_RJ)
                path.to_krj(map_loading)
        elif units == "K_RJ":
            den = torch.as_tensor(self._band_denominators(all_dets)[lo:hi].astype(np.float32), device=device)[:, None]
            for field in (map_loading, noise):
                if field is not None:
                    field /= den
        if lagged:  # the noise is the law of the readout's output and stays as drawn
            optical = [n for n, f in (("atmosphere", loading), ("map", map_loading)) if f is not None]
            self._apply_time_constants(obs, [f for f in (loading, map_loading) if f is not None], tau)
            metadata["time_constants"] = {"applied": True, "fields": optical, "init": "steady"}
        for name, field in (("atmosphere", loading), ("map", map_loading), ("noise", noise)):
            if field is not None:
                obs.loading[name] = field if self.device_output else field.cpu().numpy()
        coords = obs.coords if rows is None else obs.boresight.broadcast(obs.coords.offsets[lo:hi])
        tod = TOD(data=obs.loading, dets=dets, coords=coords, units=units, metadata=metadata)
        tod._calibrator = self._make_calibrator(obs, metadata, (lo, hi))
        if units_out != units:
            tod = tod.to(units_out)
            obs.loading = tod.data
        return tod

    def _sample_hwp(self, obs, rows, dets):
        """The map field behind the half-wave plate, [D, T] pW: S_I + S_c cos 4 chi + S_s sin 4 chi from three passes of
        the sampler -- the detectors' I weights alone, the Q / U weights of angle -gamma, those of pi / 4 - gamma --
        combined in place by ``mrx_tod_hwp_modulate``.  A map without Q and U has S_c = S_s = 0: one pass, no launch."""
        import torch

        from . import hwp as mhwp
        from . import map as mmap
        from ._lib import Context

        rows_i = np.zeros((dets.n, 4))
        rows_i[:, 0] = mmap.mueller_row(dets.gamma)[:, 0]
        out = self._sample_maps(obs, rows, stokes_rows=rows_i)
        if not set(self.map.stokes) & {"Q", "U"}:
            return out
        fields = []
        for g in (-dets.gamma, np.pi / 4 - dets.gamma):
            w = mmap.mueller_row(g)
            w[:, 0] = w[:, 3] = 0.0
            fields.append(self._sample_maps(obs, rows, stokes_rows=w))
        if hasattr(obs, "atmosphere"):
            path = obs.atmosphere._device_path()
            ctx, device = path.ctx, path.device
        else:
            device = torch.device(self.device)
            self._noise_ctx = self._noise_ctx or Context(device.index or 0)
            ctx = self._noise_ctx
        ctx.set_stream(torch.cuda.current_stream(device))
        return mhwp.modulate(out, fields[0], fields[1], mhwp.carrier(self.hwp.angle(obs.coords.t)), out=out, ctx=ctx)

    @staticmethod
    def _time_constants(dets):
        """[D] seconds, the time constants of ``dets``, or None where every one is 0: no launch, no metadata key and the
        bits of a run without them."""
        tau = np.asarray(dets.time_constant, float)
        return tau if np.any(tau > 0) else None

    def _apply_time_constants(self, obs, fields, tau):
        """``mrx_tod_onepole`` from the steady state over each of ``fields`` ([D, T] float32 pW on the device), in place:
        every row through its detector's one-pole lag ``tau`` [D] (seconds) at the rate of the observation's samples."""
        import torch

        from . import time_constants
        from ._lib import Context

        if hasattr(obs, "atmosphere"):
            path = obs.atmosphere._device_path()
            ctx, device = path.ctx, path.device
        else:
            device = torch.device(self.device)
            self._noise_ctx = self._noise_ctx or Context(device.index or 0)
            ctx = self._noise_ctx
        ctx.set_stream(torch.cuda.current_stream(device))
        a = torch.as_tensor(time_constants.poles(tau, time_constants.sample_rate_of(obs.coords.t))).to(device)
        for field in fields:
            time_constants.apply(field, a, init="steady", out=field, ctx=ctx)

    @staticmethod
    def _band_denominators(dets):
        """Without an atmosphere the transmission integral of ``TOD.to("K_RJ")`` is the band's own
        Int passband dnu, one number per band (band/band.py:246-248, calibration/functions.py:73-90):
        pW per K_RJ for every detector row."""
        den = np.empty(dets.n)
        for b, band in enumerate(dets.bands):
            rows = dets.band_index == b
            polarized = bool((~np.isnan(dets.gamma[rows])).all()) if rows.any() else False
            den[rows] = (0.5 if polarized else 1.0) * 1e12 * 1.380649e-23 * float(np.trapezoid(band.passband(band.nu), x=band.nu))
        return den

    def _make_calibrator(self, obs, metadata, rows):
        """What ``TOD.to`` needs to move a finished TOD between pW and K_RJ: the observation's
        calibration on the device (atmosphere) or one number per band (none)."""
        lo, hi = rows
        has_atm = hasattr(obs, "atmosphere")

        def convert(data, to_krj):
            import torch

            out = {}
            if has_atm:
                path = obs.atmosphere._device_path()
                self._set_calibration(obs, metadata)
                device = path.device
            else:
                device = torch.device(self.device)
                den = self._band_denominators(obs.instrument.dets)[lo:hi]
            for name, field in data.items():
                on_device = isinstance(field, torch.Tensor)
                f = (field.clone() if on_device else torch.as_tensor(np.ascontiguousarray(field, np.float32)).to(device)).contiguous()
                if has_atm:
                    path.to_krj(f) if to_krj else path.from_krj(f)
                else:
                    d = torch.as_tensor(den.astype(np.float32), device=f.device)[:, None]
                    f = f / d if to_krj else f * d
                out[name] = f if on_device else f.cpu().numpy()
            return out

        return convert
