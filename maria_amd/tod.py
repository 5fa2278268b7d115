"""``TOD``: the data container with its time-domain cleaning chain, and the ``Coordinates`` it carries.

Mirrors the slice of ``maria.tod.TOD`` and ``maria.coords.Coordinates`` the device path fills.  Neither the simulation
driver nor the atmosphere is imported here, and torch and ``_lib`` only inside the functions: this module loads where no
device and no library is."""

from __future__ import annotations

import numpy as np

from . import _tod_args

HALF_PI_F32 = np.float32(np.pi / 2)


def _tensor(v):
    import torch

    return v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


def field_device(fields, device):
    """The device that takes a TOD's ``fields``: the first field's own, or ``device`` where that field is on the host."""
    import torch

    v = _tensor(next(iter(fields)))
    return v.device if v.is_cuda else torch.device(device)


def field_sum(fields, dev):
    """The sum of ``fields`` as a contiguous float32 tensor on ``dev``: the first field cloned, the rest added in order
    (what makes the sum's bits).  No per-field copy is kept."""
    import torch

    signal = None
    for v in fields:
        v = _tensor(v).to(dev, torch.float32)
        signal = v.clone() if signal is None else signal.add_(v)
    return signal.contiguous()


def check_bounds_array(bounds, T):
    """[S + 1] int32 segment bounds from an ascending integer array, clamped to 0 .. T."""
    bounds = np.asarray(bounds)
    if bounds.ndim != 1 or bounds.size < 2 or bounds.dtype.kind not in "iu" or np.any(np.diff(bounds.astype(np.int64)) < 0):
        raise ValueError("bounds must be a one-dimensional array of S + 1 >= 2 ascending integers")
    return np.clip(bounds.astype(np.int64), 0, T).astype(np.int32)


def check_factor(q):
    from .downsample import MAX_FACTOR, MIN_FACTOR

    if int(q) != q or not MIN_FACTOR <= int(q) <= MAX_FACTOR:
        raise ValueError(f"q {q}: an integer in {MIN_FACTOR} .. {MAX_FACTOR}")
    return int(q)


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

    @property
    def _T(self):
        return int(np.asarray(self.coords.t).size)

    def _sample_rate(self):
        """(n - 1) / (t[-1] - t[0]), unguarded: every caller says itself what fewer than two samples mean."""
        t = np.asarray(self.coords.t, float)
        return (t.size - 1) / (t[-1] - t[0])

    def _derived(self, data=None, flags=None, coords=None, dets=None, units=None, record=None):
        """A TOD derived from this one: every argument left None is this TOD's own object, and the pW <-> K_RJ calibrator
        is carried over.  ``record``: metadata keys the step adds to a shallow copy of the metadata; None shares the
        dict itself."""
        own = lambda v, mine: mine if v is None else v  # noqa: E731
        out = TOD(data=own(data, self.data), dets=own(dets, self.dets), coords=own(coords, self.coords), units=own(units, self.units),
                  metadata=self.metadata if record is None else {**self.metadata, **record}, flags=own(flags, self.flags))
        out._calibrator = getattr(self, "_calibrator", None)
        return out

    def _signal(self, device, field=None):
        """The sum of the fields (or the one ``field``) on the device that takes this TOD's fields, nothing else kept."""
        fields = list(self.data.values())
        return field_sum(fields if field is None else [self.data[field]], field_device(fields, device))

    def _field_copies(self, device):
        """(data, signal, dev): float32 contiguous copies of every field on ``dev``, the first field's device (a host
        field: ``device``), and their sum.  Nothing is checked against the coordinates."""
        import torch

        dev = field_device(self.data.values(), device)
        data, signal = {}, None
        for name, v in self.data.items():
            data[name] = _tensor(v).to(dev, torch.float32, copy=True).contiguous()
            signal = data[name].clone() if signal is None else signal.add_(data[name])
        return data, signal, dev

    def _field_views(self, device):
        """(data, dev): every field as float32 on ``dev`` (as in ``_field_copies``) without a copy where none is needed:
        a field is made contiguous only if its stride along time is not 1, so a padded row pitch stays and a float32
        device field is the caller's own tensor.  For ``downsample`` and ``demodulate``, which only read."""
        import torch

        dev = field_device(self.data.values(), device)
        data = {}
        for name, v in self.data.items():
            x = _tensor(v).to(dev, torch.float32)
            data[name] = x.contiguous() if x.dim() == 2 and x.shape[1] > 1 and x.stride(1) != 1 else x
        return data, dev

    def _operands(self, signal, model, ctx):
        """(model, flags, ctx) beside ``signal``: the signal's shape checked against the coordinates, then the model's
        against the signal's; model and flags on the signal's device, and a context made for the call if none is given."""
        import torch

        T = self._T
        if tuple(signal.shape) != (signal.shape[0], T):
            raise ValueError(f"fields of shape {tuple(signal.shape)}: the coordinates have {T} samples")
        if model is not None:
            model = _tensor(model)
            if tuple(model.shape) != tuple(signal.shape):
                raise ValueError(f"model of shape {tuple(model.shape)}: the fields' {tuple(signal.shape)}")
            model = model.to(signal.device, torch.float32).contiguous()
        flags = None if self.flags is None else torch.as_tensor(self.flags).to(signal.device, torch.uint8).contiguous()
        return model, flags, _tod_args.context(ctx, signal)

    def _device_fields(self, model, into, ctx, device):
        """(data, signal, model, flags, into, ctx) for ``remove_ground``, ``regress``, ``remove_common_mode`` and the like: float32
        device copies of the fields, their sum, the model and the flags on the same device.  It refuses a bad ``into``
        first, then fields that do not match the coordinates, then a model of another shape."""
        into = self.fields[0] if into is None else into
        if into not in self.data:
            raise ValueError(f"into {into!r}: one of the fields {self.fields}")
        data, signal, _ = self._field_copies(device)
        model, flags, ctx = self._operands(signal, model, ctx)
        return data, signal, model, flags, into, ctx

    def _groups(self, groups, dtype):
        """``groups`` of ``remove_common_mode`` and ``cut`` as an integer array of ``dtype``, or None: "band"
        (``dets.band_index``), None (one group) or an integer array with entries >= -1."""
        if isinstance(groups, str):
            if groups != "band":
                raise ValueError(f'groups {groups!r}: "band", None or an integer array')
            return np.asarray(self.dets.band_index, dtype)
        if groups is None:
            return None
        groups = np.asarray(groups)
        if groups.ndim != 1 or groups.dtype.kind not in "iu" or (groups.size and groups.min() < -1):
            raise ValueError("groups must be a one-dimensional integer array with entries >= -1")
        return groups.astype(dtype)

    def _hwp(self, hwp):
        """``hwp``, or the half-wave plate the simulation recorded in ``metadata["hwp"]``."""
        if hwp is not None:
            return hwp
        from .hwp import HWP

        if "hwp" not in self.metadata:
            raise ValueError('no hwp given and no metadata["hwp"]: this TOD was not simulated behind a half-wave plate')
        return HWP.from_metadata(self.metadata["hwp"])

    def _radius(self, radius, degrees, allow_zero):
        """``radius`` in radians (None: 3 x the largest beam FWHM of the detector table), finite and positive, or 0 with
        ``allow_zero``."""
        if radius is None:
            radius = 3.0 * float(self.beam_fwhm().max())
        else:
            radius = float(radius) * (np.pi / 180 if degrees else 1.0)
        if not (np.isfinite(radius) and (radius >= 0 if allow_zero else radius > 0)):
            raise ValueError(f"radius {radius}: finite and {'>=' if allow_zero else '>'} 0")
        return radius

    def _every_qth(self, q, rows=None):
        """(coords, flags) of this TOD reduced by ``q``: the boresight and the times picked at every q-th sample and
        ``flagging.downsample_flags(flags, q)``; ``rows``: the detector rows of the result (``demodulate`` repeats them)."""
        c = self.coords
        offsets = c.offsets if rows is None or c.offsets is None else c.offsets[rows]
        coords = Coordinates(np.asarray(c.t, float)[::q], c._baz[::q], c._bel[::q], offsets=offsets)
        flags = self.flags
        if flags is not None:
            import torch

            from .flagging import downsample_flags

            flags = downsample_flags(flags if rows is None else torch.as_tensor(flags), q)  # (demodulate takes host flags too)
            if rows is not None:
                flags = flags.index_select(0, torch.as_tensor(rows).to(flags.device))
        return coords, flags

    def psd(self, nperseg=None, field=None, ctx=None, device="cuda:0"):
        """The Welch spectrum of every detector's row of ``field`` (default: the signal, the sum of the fields) on the
        device: ``(f, psd)``, maria_amd.noise_estimate.welch."""
        from .noise_estimate import welch

        fields = [self.data[field]] if field is not None else list(self.data.values())
        return welch(field_sum(fields, field_device(fields, device)), self._sample_rate(), nperseg=nperseg, ctx=ctx)

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
        from .downsample import decimate, design_taps, upload_taps

        q = check_factor(q)
        h = design_taps(q) if taps is None else np.ascontiguousarray(_tod_args.to_numpy(taps), np.float64)
        fields, dev = self._field_views(device)
        d_taps = upload_taps(h, dev)  # the taps go to the device once, and one context serves every field
        data = {}
        for name, x in fields.items():
            ctx = _tod_args.context(ctx, x)
            data[name] = decimate(x, q, taps=h, ctx=ctx, device_taps=d_taps)
        coords, flags = self._every_qth(q)
        rate = self._sample_rate() / q if self._T > 1 else float("nan")
        metadata = dict(self.metadata, downsample={"factor": q, "n_taps": int(h.size), "sample_rate": float(rate)})
        # (not _derived: the calibrator closes over full-rate tables and is deliberately dropped, with demodulate's)
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
        from .downsample import MAX_FACTOR

        if "demodulate" in self.metadata or "downsample" in self.metadata:
            raise ValueError("demodulate takes the TOD at the rate the half-wave plate modulated it: this one is already reduced")
        hwp = self._hwp(hwp)
        t = np.asarray(self.coords.t, float)
        if t.size < 2:
            raise ValueError("demodulate needs at least two samples to know the sample rate")
        fs = self._sample_rate()
        if q is None:
            q = min(MAX_FACTOR, mhwp.max_factor(fs, hwp.frequency))
        q = check_factor(q)
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
        fields, dev = self._field_views(device)
        d_carrier = torch.as_tensor(c).to(dev)  # the carrier goes to the device once, and one context serves every field
        data = {}
        for name, x in fields.items():
            ctx = _tod_args.context(ctx, x)
            y = torch.empty((D + 2 * Dp, T_out), dtype=torch.float32, device=dev)
            if Dp == D:  # every detector has Q and U rows: the three outputs are the three blocks of the field
                mhwp.demodulate(x, d_carrier, q, ht, hp, ctx=ctx, out=(y[:D], y[D:2 * D], y[2 * D:]))
            else:
                _, yq, yu = mhwp.demodulate(x, d_carrier, q, ht, hp, ctx=ctx, out=(y[:D], *torch.empty((2, D, T_out), dtype=torch.float32, device=dev)))
                rows = torch.as_tensor(pol).to(dev)
                y[D:D + Dp] = yq.index_select(0, rows)
                y[D + Dp:] = yu.index_select(0, rows)
            data[name] = y
        coords, flags = self._every_qth(q, rows=np.concatenate([np.arange(D), pol, pol]))
        metadata = dict(self.metadata, demodulate={"f_hwp": hwp.frequency, "factor": q, "n_taps": int(hp.size), "sample_rate": float(fs / q),
                                                   "rows": {"T": (0, D), "Q": (D, D + Dp), "U": (D + Dp, D + 2 * Dp)}})
        # (not _derived: like downsample, the result deliberately drops the pW <-> K_RJ calibrator)
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
        hwp = self._hwp(hwp)
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

        from .flagging import find_glitches, gap_fill

        data, signal, dev = self._field_copies(device)
        ctx = _tod_args.context(ctx, signal)
        flags, count = find_glitches(signal, n_sigma=n_sigma, half_window=half_window, grow=grow, ctx=ctx)
        del signal
        if self.flags is not None:
            flags |= torch.as_tensor(self.flags).to(dev, torch.uint8)
            count = (flags != 0).sum(dim=1)
        if fill:
            for x in data.values():
                gap_fill(x, flags, n_fit=n_fit, ctx=ctx)
        counts = count.cpu().numpy().astype(np.int64)
        record = {"n_sigma": float(n_sigma), "half_window": int(half_window), "grow": (int(grow[0]), int(grow[1])), "n_fit": int(n_fit),
                  "fill": bool(fill), "flagged_fraction": float(counts.sum() / flags.numel()), "counts": counts}
        return self._derived(data=data, flags=flags, record={"glitches": record})

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
        record = {"window": w, "n_sigma": float(n_sigma), "gap": g, "sep": sep, "grow": grow, "min_count": m, "n_fit": int(n_fit),
                  "fill": bool(fill), "into": into, "counts": count.cpu().numpy().astype(np.int64),
                  "positions": [ps[a:b] for a, b in zip(rs[:-1], rs[1:])], "heights": [hs[a:b] for a, b in zip(rs[:-1], rs[1:])],
                  "unfixed": int((~ok).sum()), "flagged_fraction": float((jump_flags != 0).sum()) / jump_flags.numel()}
        return self._derived(data=data, flags=jump_flags, record={"jumps": record})

    def remove_lines(self, lines=None, chunk=None, n_poly=2, n_sigma=6.0, nperseg=None, n_refine=2, per_detector=True, groups="band",
                     model=None, into=None, min_hits=None, rcond=1e-10, ctx=None, device="cuda:0"):
        """A new TOD with narrow spectral lines (pulse-tube lines and their harmonics, aliased mains, microphonic
        resonances) found, tracked per detector and subtracted (maria_amd.lines).  The lines are those of
        ``lines``, frequencies in Hz ([L], or [D, L] per detector), or with None the ones ``lines.find_lines`` reports
        above ``n_sigma`` robust sigmas in the Welch spectrum (:meth:`psd`'s, ``nperseg`` samples a segment) of the signal
        (the sum of the fields, less ``model``) of every group of detectors (``groups``: "band", None for one group, or an
        integer array, -1: a detector left as it is).  In ascending frequency, three neighbours at a time (each set on the
        signal the earlier sets are already gone from): every detector's frequencies are tracked by ``n_refine`` rounds of
        the phase slope between consecutive chunks (``lines.refine``; ``per_detector`` False: one correction a group),
        then each chunk of ``chunk`` seconds (None: ``nperseg`` samples) gets an amplitude and a phase per line beside
        ``n_poly`` (0 .. 2) Legendre baseline terms, and the carriers alone are subtracted from the field ``into``
        (default: the first; the mappers bin the sum).  With lines from the finder the chunks must not be longer than
        ``nperseg`` samples: a frequency known to half a Welch bin must not slip half a cycle from one chunk to the next.
        Samples with nonzero ``flags`` take no part in the fits, and are subtracted from like the rest.  A (detector,
        chunk) pair with fewer than max(min_hits, K) samples left (``min_hits`` None: 4 K, K = n_poly + 2 lines of the
        set), or whose basis is degenerate on them, is left as it is and counted.  Run it after ``flag_glitches`` and
        ``fix_jumps`` (a spike or a step is broadband and leaks into every line) and before ``cut_uncorrelated``,
        ``remove_ground`` and ``remove_common_mode`` (a line common to the array would otherwise enter their templates).
        Every field of the result is a float32 device copy; ``flags``, ``dets``, ``coords``, ``units`` and the pW <-> K_RJ
        calibrator are carried over; ``metadata["lines"]`` records the parameters, ``bounds``, the ``found`` and ``refined``
        frequencies ([D, L] in Hz, strongest first, NaN where a detector's group has fewer lines), the per-chunk
        ``amplitude`` and ``phase`` ([D, S, L]) and the ``unfitted`` count.  A TOD without lines comes back with every bit
        of its fields.  This TOD is left as it is."""
        import torch

        from . import lines as mlines
        from .cuts import chunk_bounds
        from .noise_estimate import check_nperseg, default_nperseg, welch

        n_poly = mlines._check_n_poly(n_poly)
        if min_hits is not None:
            min_hits = _tod_args.check_min_hits(min_hits)
        if not 0.0 <= float(rcond) < 1.0:
            raise ValueError(f"rcond {rcond}: in [0, 1)")
        if isinstance(n_refine, bool) or int(n_refine) != n_refine or int(n_refine) < 0:
            raise ValueError(f"n_refine {n_refine}: an integer >= 0")
        if not (np.isfinite(float(n_sigma)) and float(n_sigma) > 0):
            raise ValueError(f"n_sigma {n_sigma}: finite and > 0")
        T = self._T
        if T < 2:
            raise ValueError("a TOD of fewer than two samples has no sample rate")
        fs = float(self._sample_rate())
        nperseg = default_nperseg(T) if nperseg is None else check_nperseg(nperseg, T)
        if chunk is not None and not (np.isfinite(float(chunk)) and round(float(chunk) * fs) >= 1):
            raise ValueError(f"chunk {chunk}: a finite number of seconds, at least one sample")
        length = nperseg if chunk is None else int(round(float(chunk) * fs))
        if lines is None and length > nperseg:
            raise ValueError(f"chunks of {length} samples with lines from the finder: at most nperseg = {nperseg}")
        group = self._groups(groups, np.int64)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        D = int(signal.shape[0])
        group = np.zeros(D, np.int64) if group is None else group
        if group.shape != (D,):
            raise ValueError(f"groups must be {D} integers, one per detector")
        G = int(group.max()) + 1 if group.size and group.max() >= 0 else 0
        if model is not None:
            signal.sub_(model)
        if lines is None:
            f, p = welch(signal, fs, nperseg=nperseg, ctx=ctx)
            found = mlines.find_lines(f.cpu().numpy(), p.cpu().numpy(), groups=group, n_sigma=n_sigma)
            per_row = None
        else:
            hz = np.asarray(_tod_args.to_numpy(lines), np.float64)
            if hz.ndim not in (1, 2) or hz.shape[-1] < 1 or (hz.ndim == 2 and hz.shape[0] != D) or not np.all(np.isfinite(hz)) \
                    or not (np.all(hz > 0) and np.all(hz <= 0.5 * fs)):
                raise ValueError(f"lines must be [L] or [{D}, L] frequencies in (0, {0.5 * fs}] Hz, L >= 1")
            per_row = hz if hz.ndim == 2 else None
            found = [hz.mean(axis=0) if hz.ndim == 2 else hz] * G
        bounds = chunk_bounds(T, length)
        S = bounds.size - 1
        d_bounds = torch.as_tensor(bounds).to(signal.device)
        Lmax = max([v.size for v in found] + [0])
        rec_found, rec_refined = np.full((D, Lmax), np.nan), np.full((D, Lmax), np.nan)
        amplitude, phase = np.full((D, S, Lmax), np.nan), np.full((D, S, Lmax), np.nan)
        unfitted = 0
        nonempty = torch.as_tensor(np.diff(bounds.astype(np.int64)) > 0).to(signal.device)
        for k, freqs in enumerate(found):
            rows = np.flatnonzero(group == k)
            if rows.size == 0 or freqs.size == 0:
                continue
            whole = rows.size == D
            d_rows = torch.as_tensor(rows).to(signal.device)
            work = signal if whole else signal.index_select(0, d_rows)
            target = data[into] if whole else data[into].index_select(0, d_rows)
            fl = flags if flags is None or whole else flags.index_select(0, d_rows)
            start = np.broadcast_to(freqs[None, :], (rows.size, freqs.size)) if per_row is None else per_row[rows]
            rec_found[np.ix_(rows, np.arange(freqs.size))] = start
            order = np.argsort(freqs)
            for members in mlines.line_groups(freqs.size):
                cols = order[list(members)]
                K = n_poly + 2 * cols.size
                mh = 4 * K if min_hits is None else min_hits
                nu = mlines.refine(work, d_bounds, start[:, cols] / fs, n_iter=int(n_refine), per_detector=per_detector, n_poly=n_poly, flags=fl,
                                   min_hits=mh, rcond=rcond, ctx=ctx)
                a, ok = mlines.fit(work, d_bounds, nu, n_poly=n_poly, flags=fl, min_hits=mh, rcond=rcond, ctx=ctx)
                mlines.apply(work, d_bounds, nu, a, n_poly, sign=-1, out=work, ctx=ctx)
                mlines.apply(target, d_bounds, nu, a, n_poly, sign=-1, out=target, ctx=ctx)
                amp, phi = mlines.amplitude_phase(a, n_poly)
                rec_refined[np.ix_(rows, cols)] = nu * fs
                amplitude[np.ix_(rows, np.arange(S), cols)] = amp.cpu().numpy()
                phase[np.ix_(rows, np.arange(S), cols)] = phi.cpu().numpy()
                unfitted += int((~ok & nonempty[None, :]).sum())
            if not whole:
                data[into].index_copy_(0, d_rows, target)
        del signal
        record = {"n_poly": n_poly, "n_sigma": float(n_sigma), "nperseg": nperseg, "chunk": None if chunk is None else float(chunk),
                  "n_refine": int(n_refine), "per_detector": bool(per_detector), "min_hits": min_hits, "rcond": float(rcond), "into": into,
                  "bounds": bounds, "lines": [np.array(v, np.float64) for v in found], "found": rec_found, "refined": rec_refined,
                  "amplitude": amplitude, "phase": phase, "unfitted": unfitted}
        return self._derived(data=data, record={"lines": record})

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
        lo = hi = None
        if bins is None:
            bins, lo, hi = ground.azimuth_bins(self.coords._baz, n_bins)
        bins = ground._check_bins(bins, n_bins, self._T)
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
        record = {"n_bins": n_bins, "lo": lo, "hi": hi, "min_hits": int(min_hits), "shared": bool(shared), "empty_bins": empty,
                  "template": template.cpu().numpy()}
        return self._derived(data=data, record={"ground": record})

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
        B = _tensor(templates)
        T = self._T
        if B.dim() != 2 or B.shape[1] != T or not 1 <= B.shape[0] <= regress.MAX_TEMPLATES:
            raise ValueError(f"templates must be a [K, {T}] array with K in 1 .. {regress.MAX_TEMPLATES}")
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        B = B.to(signal.device, torch.float32).contiguous()[None]
        N, r, hits = regress.normal_equations(signal, B, flags=flags, model=model, ctx=ctx)
        del signal
        a, ok = regress.solve(N, r, hits, min_hits=min_hits, rcond=rcond)
        regress.apply(data[into], B, a, sign=-1, out=data[into], ctx=ctx)
        record = {"n_templates": int(B.shape[1]), "min_hits": min_hits, "rcond": float(rcond), "coefficients": a.cpu().numpy(),
                  "failed_rows": np.flatnonzero(~ok.cpu().numpy())}
        return self._derived(data=data, record={"regress": record})

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
        groups = self._groups(groups, np.int32)
        G =1 if groups is None or not groups.size else max(int(groups.max()) + 1, 1)
        _tod_args.check_count(G, "the number of groups", regress.MAX_GROUPS)
        if int(poly_order) != poly_order or int(poly_order) < 0 or 2 + int(poly_order) + bool(airmass) > regress.MAX_TEMPLATES:
            raise ValueError(f"poly_order {poly_order}: an integer >= 0 with 2 + poly_order + airmass <= {regress.MAX_TEMPLATES}")
        extra = [regress.legendre_templates(self._T, int(poly_order))[1:]]
        if airmass:
            extra.append(regress.airmass_template(self.coords._bel)[None])
        extra = np.concatenate(extra)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        c, a, gains, ok, B = regress.fit_common_mode(signal, groups=groups, n_groups=G, flags=flags, model=model,
                                                     extra=extra if extra.shape[0] else None, n_iter=n_iter, min_hits=min_hits,
                                                     rcond=rcond, ctx=ctx)
        del signal
        regress.apply(data[into], B, a, groups=groups, sign=-1, out=data[into], ctx=ctx)
        a_host = a.cpu().numpy()
        grouped = np.ones(a_host.shape[0], bool) if groups is None else groups >= 0  # a detector left out has not failed
        record = {"n_groups": G, "n_iter": int(n_iter), "poly_order": int(poly_order), "airmass": bool(airmass), "min_hits": min_hits,
                  "rcond": float(rcond), "gains": gains.cpu().numpy(), "offsets": a_host[:, 0].copy(), "coefficients": a_host,
                  "common_mode": c.cpu().numpy(), "failed_rows": np.flatnonzero(~ok.cpu().numpy() & grouped)}
        return self._derived(data=data, record={"common_mode": record})

    def remove_sky_polynomial(self, order=1, groups="band", n_iter=3, min_hits=8, min_dets=None, rcond=1e-10, flag_failed=True, model=None,
                              into=None, ctx=None, device="cuda:0"):
        """A new TOD with a planar (``order`` 1) or quadratic (2) sky surface removed sample by sample
        (maria_amd.sky_polynomial; Sayers et al. 2010); in ``remove_common_mode``'s place in the chain, which
        is its ``order`` 0.  Per group of detectors (``groups`` as in :meth:`remove_common_mode`) and at every sample a
        polynomial in the detectors' focal-plane offsets (``sky_polynomial.basis`` of ``dets.offsets``: K = 1, 3 or 6
        terms) is fitted by gain-weighted least squares to the signal (the sum of the fields, less ``model``) of the
        detectors whose flag is 0 there, and y = x - (o_d + g_d sum_k c_k(t) P_dk) is taken from the field ``into``
        (default: the first).  The gains g and offsets o are those of ``regress.fit_common_mode`` (``n_iter``,
        ``min_hits`` samples a detector, ``rcond``); a detector whose fit failed there is left as it is and takes no part.
        A sample with fewer than ``min_dets`` (None: 2 K) detectors left, or whose terms are degenerate on them
        (``regress.solve``'s verdict with ``rcond``), has only the offset removed and, with ``flag_failed``, is flagged
        in the group's rows.  Flagged samples take part in no sum and are subtracted from like the rest.  Every field of
        the result is a float32 device copy; ``dets``, ``coords``, ``units`` and the pW <-> K_RJ calibrator are carried
        over; ``metadata["sky_polynomial"]`` records ``order``, ``n_terms``, ``n_groups``, ``n_iter``, ``min_hits``,
        ``min_dets``, ``rcond``, ``flag_failed``, the [D] ``gains`` and ``offsets``, the [G, K, T] float64
        ``coefficients``, ``failed_rows`` and the [n, 2] (group, sample) ``failed_samples``.  This TOD is left as it is."""
        import torch

        from . import sky_polynomial

        K = sky_polynomial.n_terms(order)
        min_hits = _tod_args.check_min_hits(min_hits)
        n_iter = _tod_args.check_count(n_iter, "n_iter", 64)
        if not 0.0 <= float(rcond) < 1.0:
            raise ValueError(f"rcond {rcond}: in [0, 1)")
        groups = self._groups(groups, np.int32)
        G = 1 if groups is None or not groups.size else max(int(groups.max()) + 1, 1)
        _tod_args.check_count(G, "the number of groups", sky_polynomial.MAX_GROUPS)
        min_dets = 2 * K if min_dets is None else min_dets
        if isinstance(min_dets, bool) or int(min_dets) != min_dets or int(min_dets) < 1:
            raise ValueError(f"min_dets {min_dets}: None or an integer >= 1")
        offsets = np.asarray(self.dets.offsets, np.float64)
        if groups is not None and groups.shape[0] != offsets.shape[0]:
            raise ValueError(f"groups must have one entry for each of the {offsets.shape[0]} detectors")
        P_host = sky_polynomial.basis(offsets, int(order), groups=groups, n_groups=G)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        D, T = signal.shape
        if D != P_host.shape[0]:
            raise ValueError(f"fields of {D} rows: the detector table has {P_host.shape[0]}")
        dev = signal.device
        P = torch.as_tensor(P_host).to(dev)
        c, ok_t, gains, offs, ok_d = sky_polynomial.fit_sky(signal, P, groups=groups, n_groups=G, flags=flags, model=model, n_iter=n_iter,
                                                            min_hits=min_hits, min_dets=int(min_dets), rcond=rcond, ctx=ctx)
        del signal
        d_groups = torch.zeros(D, dtype=torch.int32, device=dev) if groups is None else torch.as_tensor(groups).to(dev)
        fitted = torch.where(ok_d, d_groups, torch.full_like(d_groups, -1))  # a detector without gain and offset is copied
        sky_polynomial.apply(data[into], P, c, gains, e=offs, groups=fitted, sign=-1, out=data[into], ctx=ctx)
        new_flags = flags
        if flag_failed:
            inside = (d_groups >= 0) & (d_groups < G)
            failed = ~ok_t[torch.where(inside, d_groups, torch.zeros_like(d_groups)).to(torch.int64)] & inside[:, None]  # [D, T]
            new_flags = failed.to(torch.uint8) if flags is None else flags | failed.to(torch.uint8)
        grouped = np.ones(D, bool) if groups is None else groups >= 0  # a detector left out has not failed
        record = {"order": int(order), "n_terms": K, "n_groups": G, "n_iter": int(n_iter), "min_hits": min_hits, "min_dets": int(min_dets),
                  "rcond": float(rcond), "flag_failed": bool(flag_failed), "gains": gains.cpu().numpy(), "offsets": offs.cpu().numpy(),
                  "coefficients": c.cpu().numpy(), "failed_rows": np.flatnonzero(~ok_d.cpu().numpy() & grouped),
                  "failed_samples": np.argwhere(~ok_t.cpu().numpy())}
        return self._derived(data=data, flags=new_flags, record={"sky_polynomial": record})

    def _covariance_groups(self, groups, D):
        """(groups as [D] int32 or None, their number) for the covariance methods: at most 16 groups."""
        from . import covariance

        groups = self._groups(groups, np.int32)
        if groups is not None and groups.shape[0] != D:
            raise ValueError(f"groups must have one entry for each of the {D} detectors")
        G = 1 if groups is None or not groups.size else max(int(groups.max()) + 1, 1)
        return groups, _tod_args.check_count(G, "the number of groups", covariance.MAX_GROUPS)

    def covariance(self, groups="band", field=None, model=None, min_hits=8, ctx=None, device="cuda:0"):
        """``(tod, cov)``: the flag-aware covariance between the detectors of each group (maria_amd.covariance.covariance,
        DESIGN 3.34) of the signal (the sum of the fields, or the one ``field``; less ``model``) over the samples whose
        ``flags`` are 0, and this TOD with ``metadata["covariance"]`` recording ``n_groups``, ``min_hits``, ``field`` and
        per group the ``rows``, the number of ``unusable`` rows and the largest eigenvalue's share of the usable
        correlation matrix' trace.  ``groups``: "band", None (one group) or an integer array, -1 leaving a detector
        out (at most 16 groups).  Nothing of this TOD is copied or changed."""
        from . import covariance

        min_hits = _tod_args.check_min_hits(min_hits)
        if field is not None and field not in self.data:
            raise ValueError(f"field {field!r}: one of the fields {self.fields}")
        signal = self._signal(device, field)
        groups, G = self._covariance_groups(groups, signal.shape[0])
        model, flags, ctx = self._operands(signal, model, ctx)
        cov = covariance.covariance(signal, groups=groups, n_groups=G, flags=flags, model=model, min_hits=min_hits, ctx=ctx)
        per_group = []
        for cg in cov.groups:
            usable = int((~cg.unusable).sum())
            share = float(covariance.leading_modes(cg, 1)[0][0]) / usable if usable else float("nan")
            per_group.append({"rows": cg.rows.cpu().numpy(), "unusable": int(cg.unusable.sum()), "leading_share": share})
        record = {"n_groups": G, "min_hits": min_hits, "field": field, "groups": per_group}
        return self._derived(record={"covariance": record}), cov

    def remove_modes(self, n_modes=1, groups="band", model=None, into=None, min_hits=8, rcond=1e-10, remove_mean=False, ctx=None,
                     device="cuda:0"):
        """A new TOD with the ``n_modes`` (1 .. 7) leading modes of each group's flag-aware correlation matrix removed
        (maria_amd.covariance); after ``remove_common_mode`` or in its place, before ``filter_subscans``.
        Per group of detectors (``groups`` as in :meth:`remove_common_mode`): the covariance of the signal (the sum of the
        fields, less ``model``) over the samples whose flags are 0, the leading eigenvectors of its correlation matrix
        (``covariance.leading_modes``), and per mode the time template that is the flag-aware projection of the
        normalised detectors onto the eigenvector (``covariance.mode_templates``).  Every detector is fitted to
        [1, the templates] by least squares (``regress.normal_equations``, ``regress.solve``) and the modes are subtracted
        from the field ``into`` (default: the first), the constant too only with ``remove_mean``.  Flagged samples take
        part in no sum and are subtracted from like the rest; a detector that cannot be fitted, and every detector of a
        group with fewer usable rows than modes, is left as it is.  Every field of the result is a float32 device copy;
        ``flags``, ``dets``, ``coords``, ``units`` and the calibrator are carried over; ``metadata["modes"]`` records
        ``n_modes``, ``n_groups``, ``min_hits``, ``rcond``, ``remove_mean``, the [G, n_modes] ``eigenvalues``, the
        [D, n_modes] ``loadings``, the [D, 1 + n_modes] ``coefficients``, the [G, 1 + n_modes, T] float32 ``templates``
        and ``failed_rows``.  This TOD is left as it is."""
        import torch

        from . import covariance, regress

        min_hits = _tod_args.check_min_hits(min_hits)
        n_modes = _tod_args.check_count(n_modes, "n_modes", covariance.MAX_MODES)
        data, signal, model, flags, into, ctx = self._device_fields(model, into, ctx, device)
        groups, G = self._covariance_groups(groups, signal.shape[0])
        cov = covariance.covariance(signal, groups=groups, n_groups=G, flags=flags, model=model, min_hits=min_hits, ctx=ctx)
        eig, U = covariance.loadings(cov, n_modes)
        B = torch.ones((G, 1 + n_modes, signal.shape[1]), dtype=torch.float32, device=signal.device)
        B[:, 1:, :] = covariance.mode_templates(signal, cov, U, flags=flags, model=model, ctx=ctx)
        N, r, hits = regress.normal_equations(signal, B, groups=groups, flags=flags, model=model, ctx=ctx)
        del signal
        a, ok = regress.solve(N, r, hits, min_hits=min_hits, rcond=rcond)
        sub = a if remove_mean else torch.cat([torch.zeros_like(a[:, :1]), a[:, 1:]], dim=1).contiguous()
        regress.apply(data[into], B, sub, groups=groups, sign=-1, out=data[into], ctx=ctx)
        grouped = np.ones(a.shape[0], bool) if groups is None else groups >= 0  # a detector left out has not failed
        record = {"n_modes": n_modes, "n_groups": G, "min_hits": min_hits, "rcond": float(rcond), "remove_mean": bool(remove_mean),
                  "eigenvalues": eig.cpu().numpy(), "loadings": U.cpu().numpy(), "coefficients": a.cpu().numpy(),
                  "templates": B.cpu().numpy(), "failed_rows": np.flatnonzero(~ok.cpu().numpy() & grouped)}
        return self._derived(data=data, record={"modes": record})

    def cut_uncorrelated(self, groups="band", n_sigma=5.0, min_correlation=None, min_hits=8, value=1, model=None, ctx=None,
                         device="cuda:0"):
        """``(tod, verdict)``: a new TOD whose flags also cover the detectors that do not see what their group sees
        (maria_amd.covariance); after ``fix_jumps`` / ``mask_source`` and BEFORE ``remove_ground`` /
        ``remove_common_mode``: once the common mode is out, a live detector no longer correlates with its neighbours.
        Per group (``groups`` as in :meth:`cut`) a detector's score is the median of its correlation with the other
        usable detectors (``covariance.correlation_score``) of the signal (the sum of the fields, less ``model``) over
        the samples whose flags are 0.  A detector is cut if its score is a low-side outlier of its group's
        (``cuts.find_outliers``, ``n_sigma`` robust scales below the median), if it is below ``min_correlation`` where
        one is given, or if it is unusable (fewer than max(min_hits, 1) samples kept, a constant row, a NaN; no valid
        partner).  ``value`` (1 .. 255) is ORed into the flags of every sample of a cut detector
        (``cuts.flag_segments``).  ``verdict``: the [D] float64 ``score``, the [D] bool ``outlier``, ``below``,
        ``unusable`` and ``cut`` and per group ``median`` and ``threshold`` (NaN where no scale exists), as numpy arrays;
        ``metadata["uncorrelated"]`` records it with the parameters.  Every field of the result is a float32 device
        copy, unchanged.  This TOD is left as it is."""
        import torch

        from . import covariance, cuts

        min_hits = _tod_args.check_min_hits(min_hits, allow_bool=False)
        if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= 255:
            raise ValueError(f"value {value}: an integer in 1 .. 255")
        n_sigma = float(n_sigma)
        if not np.isfinite(n_sigma) or n_sigma <= 0:
            raise ValueError(f"n_sigma {n_sigma}: finite and > 0")
        if min_correlation is not None and not -1.0 <= float(min_correlation) <= 1.0:
            raise ValueError(f"min_correlation {min_correlation}: None or in [-1, 1]")
        data, signal, model, flags, _, ctx = self._device_fields(model, None, ctx, device)
        D, T = signal.shape
        groups, G = self._covariance_groups(groups, D)
        cov = covariance.covariance(signal, groups=groups, n_groups=G, flags=flags, model=model, min_hits=min_hits, ctx=ctx)
        del signal
        verdict = covariance.judge(cov, n_sigma, min_correlation)
        new_flags = torch.zeros((D, T), dtype=torch.uint8, device=cov.mean.device) if flags is None else flags.clone()
        if bool(verdict["cut"].any()):
            cuts.flag_segments(new_flags, np.array([0, T], np.int32), verdict["cut"][:, None], value=int(value), ctx=ctx)
        verdict = {k: v.cpu().numpy() for k, v in verdict.items()}
        record = dict(verdict, n_groups=G, n_sigma=n_sigma, min_correlation=None if min_correlation is None else float(min_correlation),
                      min_hits=min_hits, value=int(value), cut_detectors=np.flatnonzero(verdict["cut"]))
        return self._derived(data=data, flags=new_flags, record={"uncorrelated": record}), verdict

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
        T = self._T
        found, turn = subscans.find_subscans(self.coords._baz, turn_frac)
        bounds = found if bounds is None else check_bounds_array(bounds, T)
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
        record = {"order": int(order), "bounds": np.array(bounds, np.int32), "turn_frac": float(turn_frac), "min_hits": min_hits,
                  "rcond": float(rcond), "coefficients": a.cpu().numpy(), "failed_segments": np.argwhere(~ok.cpu().numpy() & nonempty[None, :])}
        return self._derived(data=data, flags=new_flags, record={"subscans": record})

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
        record = dict(self.metadata.get("time_constants") or {}, deconvolved=True, deconvolved_tau=np.broadcast_to(tau, (n,)).copy(),
                      deconvolved_init=init)
        return self._derived(data=data, flags=flags, record={"time_constants": record})

    def _segment_bounds(self, bounds):
        """[S + 1] int32 bounds for ``stats`` and ``cut``, clamped to 0 .. T: None (the whole row), "subscans"
        (``subscans.find_subscans`` of the boresight azimuth), an int (chunks of that many samples) or an ascending
        integer array."""
        from . import cuts, subscans

        T = self._T
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
        return check_bounds_array(bounds, T)

    def stats(self, bounds=None, model=None, ctx=None, device="cuda:0"):
        """The statistics of the signal (the sum of the fields, less ``model``) over the samples whose ``flags`` are 0
        (maria_amd.cuts): a dict of ``bounds`` (the [S + 1] int32 segments used), ``segments`` (the
        summary of ``cuts.summarize`` per (detector, segment): [D, S] float64 device tensors ``mean``, ``var``, ``std``,
        ``skew``, ``kurtosis``, ``min``, ``max``, ``ptp``, ``sigma_diff``, ``flagged_fraction``, and int64 ``hits`` and
        ``pairs``) and ``detectors`` (the same per detector, [D], from a second pass with the row as one segment).
        ``bounds``: None (the whole row), "subscans" (``subscans.find_subscans``), an int (chunks of that many
        samples) or an ascending integer array.  This TOD is left as it is."""
        from . import cuts

        bounds = self._segment_bounds(bounds)
        signal = self._signal(device)
        model, flags, ctx = self._operands(signal, model, ctx)
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
        groups = self._groups(groups, np.int64)
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
        record = {"bounds": np.array(bounds, np.int32), "n_sigma": float(n_sigma),
                  "n_sigma_segment": None if n_sigma_segment is None else float(n_sigma_segment), "max_flagged": float(max_flagged),
                  "max_bad_segments": float(max_bad_segments), "min_hits": int(min_hits), "criteria": tuple(criteria), "value": int(value),
                  "groups": None if groups is None else groups.copy(), "masks": {k: v.cpu().numpy() for k, v in masks.items()},
                  "cut_detectors": np.flatnonzero(cut.cpu().numpy()), "cut_segments": np.argwhere((bad & ~cut[:, None]).cpu().numpy()),
                  "flagged_fraction_before": before, "flagged_fraction_after": float((new_flags != 0).sum()) / new_flags.numel()}
        return self._derived(data=data, flags=new_flags, record={"cuts": record})

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
        return self._derived(dets=dets, coords=self.coords.broadcast(offsets))

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
        T = self._T
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

        radius = self._radius(radius, degrees, allow_zero=True)
        dev = torch.device(device) if self.flags is None or not torch.as_tensor(self.flags).is_cuda else torch.as_tensor(self.flags).device
        point, center, src = self._source_frame(source, frame, src_track, degrees, dev)
        D, T = int(self.dets.n), self._T
        flags = torch.zeros((D, T), dtype=torch.uint8, device=dev) if self.flags is None else torch.as_tensor(self.flags).to(dev, torch.uint8).clone()
        beamfit.source_flags(point, center, radius, src=src, inside=True, value=value, flags=flags, ctx=ctx)
        return self._derived(flags=flags, record={"source_mask": {"center": center, "radius": radius, "frame": frame, "value": int(value)}})

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
        radius = self._radius(radius, degrees, allow_zero=False)
        signal = self._signal(device, field)
        model, flags, ctx = self._operands(signal, model, ctx)
        D, T = signal.shape
        point, center, src = self._source_frame(source, frame, src_track, degrees, signal.device)
        window = torch.zeros((D, T), dtype=torch.uint8, device=signal.device) if flags is None else (flags != 0).to(torch.uint8)
        beamfit.source_flags(point, center, radius, src=src, inside=False, value=1, flags=window, ctx=ctx)
        m = cuts.moments(signal, None, flags=window, model=model, ctx=ctx)
        mean, peak = m.mean[:, 0], m.max[:, 0]
        w0 = torch.as_tensor((beamfit.FWHM_PER_SIGMA / self.beam_fwhm()) ** 2).to(signal.device)
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
        return self._derived(data=self._calibrator(self.data, to_krj=(units == "K_RJ")), units=units)
