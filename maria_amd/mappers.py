"""``BinMapper`` (maria/mappers/bin_mapper.py): the TODs binned back onto a tangent-plane grid,
``map = ((W * D) @ P) / (W @ |P|)`` with the Stokes-weighted pointing matrix of
map/projection.py:134-179 -- on the device (``mrx_bin_map_bucketed`` / ``mrx_bin_map``), never
materialising P.  ``tod_preprocessing`` runs ``maria_amd.tod_processing.process_tod`` first, as
mappers/base.py:138 does; the map post-processing pipeline stays with maria's front end.

``MaximumLikelihoodMapper`` (maria/mappers/ml_mapper.py): the white-noise GLS map, I, Q and U solved jointly, on the
same grid and pointing, with the operators of DESIGN 3.12 (``mrx_bin_map_blocks``, ``mrx_map_block_solve``,
``mrx_map_normal_apply``).  It and ``DestripingMapper`` share one assembly loop over the TODs (``_assemble``, with
``_tod_weights`` the step the noise model decides), one solve (``_solve``) and one set of products (``_finish``)."""

from __future__ import annotations

import ctypes as C
import logging
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import destripe_prior, noise_estimate, noise_filter, noise_modes
from ._lib import Context, MrxSkyMap, ptr
from .map import ProjectionMap
from .tod import field_sum, sky_transform_stack

logger = logging.getLogger("maria")


# work buffer of the bucketed binning: all samples in one go needs 16 bytes per sample (64 bilinear); beyond this
# the call walks the time axis in chunks
BIN_WORK_LIMIT_BYTES = 24 << 30


def _work_bytes(lo, full, device):
    """The size of a routed operator's work buffer from its sizing function's minimum (one column of tiles) and full size
    (the whole time axis at once): the full size within BIN_WORK_LIMIT_BYTES and half the free memory, never below lo."""
    free = torch.cuda.mem_get_info(device)[0]
    return max(lo, min(full, BIN_WORK_LIMIT_BYTES, max(free // 2, lo)))


class TodInputs(NamedTuple):
    """One TOD on the device: the signal [D, T] a mapper bins, its per-sample weight (None for ones) and the pointing."""

    signal: torch.Tensor
    weight: torch.Tensor | None
    az: torch.Tensor
    el: torch.Tensor
    transform: torch.Tensor | None
    dx: torch.Tensor
    dy: torch.Tensor
    stokes_w: torch.Tensor
    channel: torch.Tensor

    @property
    def shape(self):
        return tuple(self.signal.shape)

    @property
    def point(self):
        """The pointing arguments of the map operators, from the boresight to the detector count."""
        D, T = self.signal.shape
        return (ptr(self.az), ptr(self.el), T, ptr(self.transform), ptr(self.dx), ptr(self.dy), ptr(self.stokes_w), ptr(self.channel), D)


def bin_map(ctx, sky, inp, msum, mwgt, bucketed=None):
    """``map_sum += (W * D) @ P``, ``map_wgt += W @ |P|`` for one TOD on the device, ``inp`` its ``TodInputs``
    (mappers/bin_mapper.py:84-120).  Maps of up to 2048 regions of 64 x 32 pixels take
    ``mrx_bin_map_bucketed`` (samples routed to map regions, summed in LDS: no scattered global
    atomics); larger ones ``mrx_bin_map`` (float64 atomics).  ``bucketed``: force (True) or
    forbid (False) the first form."""
    signal, weight = inp.signal, inp.weight
    D, T = signal.shape
    args = (C.byref(sky), ptr(signal), signal.stride(0), ptr(weight), 0 if weight is None else weight.stride(0), *inp.point,
            ptr(msum), ptr(mwgt))
    lo, full = C.c_size_t(), C.c_size_t()
    fits = ctx.lib.mrx_bin_map_work_bytes(C.byref(sky), D, T, C.byref(lo), C.byref(full)) == 0
    if bucketed is True and not fits:
        raise ValueError("the bucketed binning takes maps of at most 2048 regions of 64 x 32 pixels")
    if fits and bucketed is not False:
        work = torch.empty(_work_bytes(lo.value, full.value, signal.device), dtype=torch.uint8, device=signal.device)
        ctx.call("mrx_bin_map_bucketed", *args, ptr(work), work.numel())
        torch.cuda.current_stream(signal.device).synchronize()  # the buffer goes back to the allocator
        del work
    else:
        ctx.call("mrx_bin_map", *args)


class _AfterSubscans:
    """F = F_pre F' of one TOD: the subscan projector F' (``subscans.Projector``), then the recorded pre-processing steps
    (``tod_processing.PreprocessOperator``); the transpose in the reverse order.  In place, like its two parts."""

    def __init__(self, projector, pre):
        self.projector, self.pre = projector, pre

    def apply(self, buf):
        self.projector.apply(buf)
        return self.pre.apply(buf)

    def apply_transpose(self, buf):
        self.pre.apply_transpose(buf)
        return self.projector.apply_transpose(buf)

    def product(self):
        out = self.pre.product()
        return {**out, "steps": ["filter_subscans"] + out["steps"], "subscans": self.projector.product()}


class _GridMapper:
    """What the mappers share: the tangent-plane grid (mappers/base.py:295-301), the frame, the units, the map channels
    and, per TOD, the device inputs of the binning's pointing."""

    def _subscan_spec(self, tod):
        """The subscan filter a mapper solves through for this TOD (MaximumLikelihoodMapper's ``subscan_filter``), or None."""
        return None

    def _init_grid(self, tods, center, width, height, resolution, stokes, nu, frame, units, degrees, bilinear, tod_preprocessing,
                   device):
        self.tod_preprocessing = dict(tod_preprocessing or {})  # mappers/base.py:138: tod.process(config=...)
        if frame not in ("ra/dec", "az/el"):
            raise NotImplementedError(f"frame '{frame}': only 'ra/dec' and 'az/el' are built")
        self.tods = list(tods)
        for tod in self.tods:
            if tod.units != units:
                raise ValueError(f"the TOD is in {tod.units}; ask Simulation.run(units='{units}')")
        unit = np.pi / 180 if degrees else 1.0
        if resolution is None or (width is None and height is None):
            raise ValueError("pass 'resolution' and at least one of 'width', 'height'")
        width = height if width is None else width
        height = width if height is None else height
        self.n_xi, self.n_eta = int(max(1, width / resolution)), int(max(1, height / resolution))  # mappers/base.py:295-301
        self.xi = unit * resolution * (self.n_xi - 1) * np.linspace(-0.5, 0.5, self.n_xi)
        self.eta = (unit * resolution * (self.n_eta - 1) * np.linspace(-0.5, 0.5, self.n_eta))[::-1].copy()
        self.center = (unit * center[0], unit * center[1])
        self.resolution, self.degrees = resolution, degrees
        self.stokes, self.frame, self.units, self.bilinear = stokes, frame, units, bool(bilinear)
        self.nu = np.atleast_1d(np.asarray(150e9 if nu is None else nu, float))
        self.device = torch.device(device)
        self.products = None

    def _sky(self):
        deta, dxi = (self.eta[-1] - self.eta[0]) / (self.n_eta - 1), (self.xi[-1] - self.xi[0]) / (self.n_xi - 1)
        return MrxSkyMap(None, len(self.nu), len(self.stokes), self.n_eta, self.n_xi, float(self.eta[0]), float(deta), float(self.xi[0]),
                         float(dxi), float(self.center[0]), float(self.center[1]), 1 if self.bilinear else 0, 0)

    def _context(self):
        ctx = Context(self.device.index or 0)
        ctx.set_stream(torch.cuda.current_stream(self.device))
        return ctx

    def _tod_inputs(self, tod, ctx, unit_i_response=False, with_operator=False):
        """The ``TodInputs`` (signal, weight, az, el, transform, dx, dy, stokes_w, channel) of one TOD; weight None for ones.
        The weight is the pre-processing's window times ``tod.flags == 0`` where the TOD has flags.
        ``unit_i_response``: the Stokes weights over the detector's I weight (its Mueller [0, 0]).  ``with_operator``:
        ``(TodInputs, op)``, op the pre-processing as a ``tod_processing.PreprocessOperator`` (no steps: the identity)."""
        dev = self.device
        dets, coords = tod.dets, tod.coords
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(dev)  # noqa: E731
        weight = operator = None
        if self.tod_preprocessing or with_operator:
            from .tod_processing import preprocess_operator, process_tod

            config = {k: dict(v) for k, v in self.tod_preprocessing.items()}
            spec = self._subscan_spec(tod) if with_operator else None
            if spec is not None:  # F = F_pre F': the subscan projector first, the recorded steps on its result
                from . import subscans

                rows = field_sum(tod.data.values(), dev)
                flags = None if getattr(tod, "flags", None) is None else torch.as_tensor(tod.flags).to(dev, torch.uint8).contiguous()
                projector = subscans.Projector(rows, spec["bounds"], spec["order"] + 1, flags=flags, min_hits=spec["min_hits"],
                                               rcond=spec["rcond"], ctx=ctx)
                projector.apply(rows)
                done, operator = preprocess_operator(tod._derived(data={"total": rows}), config=config, ctx=ctx, device=dev)
                operator = _AfterSubscans(projector, operator)
            elif with_operator:
                done, operator = preprocess_operator(tod, config=config, ctx=ctx, device=dev)
            else:
                done = process_tod(tod, config=config, ctx=ctx, device=dev)
            signal = done.data["total"]
            if not np.all(done.weight == 1.0):  # the window is the processed TOD's weight (processing.py:193)
                weight = torch.as_tensor(np.ascontiguousarray(done.weight, np.float32)).to(dev).expand(signal.shape[0], -1).contiguous()
        else:
            signal = field_sum(tod.data.values(), dev)  # tod.signal, on the mapper's own device
        if getattr(tod, "flags", None) is not None:  # flagged samples get no weight (TOD.flag_glitches)
            good = (torch.as_tensor(tod.flags).to(dev) == 0).to(torch.float32)
            weight = good if weight is None else weight * good
        transform = None
        if self.frame == "ra/dec":
            transform = torch.as_tensor(sky_transform_stack(coords.t, tod.metadata["latitude"], tod.metadata["longitude"]).reshape(-1, 9)).to(dev)
        # (without an override stokes_rows() is mueller_row(dets.gamma), and its column 0 and mueller00() are both
        # 0.5 * m0 * m0: the bits of every plain detector table are what they were.  A demodulated TOD's Q and U rows
        # have no I weight of their own and divide by their detector's)
        row = dets.stokes_rows()
        if unit_i_response:
            row = row / dets.mueller00()[:, None]
        stokes_w = torch.as_tensor(np.ascontiguousarray(row[:, ["IQUV".index(s) for s in self.stokes]], np.float64)).to(dev)
        # the nu plane whose frequency is the detector's band centre, else plane 0 (projection.py:152-155)
        chan = np.zeros(dets.n, np.int32)
        for k, nu in enumerate(self.nu):
            chan[dets.band_center == nu] = k
        d_chan = torch.as_tensor(chan).to(dev)
        az, el = f32(coords._baz), f32(coords._bel)
        dx, dy = f32(coords.offsets[:, 0]), f32(coords.offsets[:, 1])
        inputs = TodInputs(signal, weight, az, el, transform, dx, dy, stokes_w, d_chan)
        return (inputs, operator) if with_operator else inputs

    def _projection_map(self, data, weight):
        out = ProjectionMap.__new__(ProjectionMap)
        out.data, out.weight = data.astype(np.float32), weight
        out.eta, out.xi, out.center = self.eta, self.xi, self.center
        unit = np.pi / 180 if self.degrees else 1.0
        out.x_res = out.y_res = unit * self.resolution
        out.stokes, out.nu, out.frame, out.units = self.stokes, self.nu, self.frame, self.units
        return out

    @property
    def map(self):
        if self.products is None:
            raise RuntimeError("Mapper has not been run yet!")
        return self.products["data"]


class BinMapper(_GridMapper):
    def __init__(self, tods, center, width=None, height=None, resolution=None, stokes="I", nu=None, frame="ra/dec",
                 units="K_RJ", degrees=True, bilinear=False, tod_preprocessing=None, map_postprocessing=None, device="cuda:0"):
        if map_postprocessing:
            # BinMapper.run overrides BaseMapper.run (mappers/bin_mapper.py:84 vs base.py:162-198):
            # the reference accepts the argument and never applies it
            logger.warning("BinMapper does not apply 'map_postprocessing' (neither does the reference's)")
        self._init_grid(tods, center, width, height, resolution, stokes, nu, frame, units, degrees, bilinear, tod_preprocessing, device)

    def run(self):
        dev = self.device
        ctx = self._context()
        S, Cn = len(self.stokes), len(self.nu)
        msum = torch.zeros((S, Cn, self.n_eta, self.n_xi), dtype=torch.float64, device=dev)
        mwgt = torch.zeros_like(msum)
        sky = self._sky()
        for tod in self.tods:
            if tod.dets.n == 0:
                continue
            bin_map(ctx, sky, self._tod_inputs(tod, ctx), msum, mwgt)
            torch.cuda.current_stream(dev).synchronize()
        data = (msum / mwgt).cpu().numpy()  # 0/0 = nan where nothing was observed, as numpy gives the reference
        self.products = {"data": data, "weight": mwgt.cpu().numpy(), "sum": msum.cpu().numpy()}
        return self._projection_map(data, self.products["weight"])


class _GlsMapper(_GridMapper):
    """What the white-noise GLS mappers share: the argument checks, the weights W, b = P^T W d with the block diagonal of
    P^T W P, the block solve and preconditioned conjugate gradients."""

    filter_aware = False  # MaximumLikelihoodMapper's keyword: ``_assemble`` then keeps every TOD's pre-processing operator

    def _init_gls(self, stokes, noise_weights, max_iter, tol, rcond, noise_fit=None):
        if not stokes or len(stokes) > 3 or any(s not in "IQU" for s in stokes) or len(set(stokes)) != len(stokes):
            raise ValueError(f"stokes '{stokes}': distinct planes of 'IQU' (the per-pixel solve takes at most three)")
        if isinstance(noise_weights, str):
            if noise_weights not in ("inverse_variance", "uniform", "fit"):
                raise ValueError(f"noise_weights '{noise_weights}': 'inverse_variance', 'uniform', 'fit' (1 / sigma^2 of the fitted "
                                 "white level) or an [ndet] array")
        else:
            noise_weights = np.asarray(noise_weights, np.float64)
            for tod in self.tods:
                if noise_weights.shape != (tod.dets.n,):
                    raise ValueError(f"noise_weights has shape {noise_weights.shape}; the TOD has {tod.dets.n} detectors")
        self.noise_weights, self.max_iter, self.tol, self.rcond = noise_weights, int(max_iter), float(tol), float(rcond)
        if noise_fit is not None:
            if not isinstance(noise_fit, dict) or set(noise_fit) - {"nperseg", "f_min", "f_max", "n_bins"}:
                raise ValueError(f"noise_fit {noise_fit!r}: a dict of 'nperseg', 'f_min', 'f_max', 'n_bins'")
            if noise_fit.get("nperseg") is not None:
                noise_estimate.check_nperseg(noise_fit["nperseg"], noise_estimate.MAX_NPERSEG)
        self.noise_fit = None if noise_fit is None else dict(noise_fit)
        self.noise_fits = []  # per TOD with detectors, when a value needs them: the fitted noise law (noise_estimate)

    def _needs_fit(self):
        return isinstance(self.noise_weights, str) and self.noise_weights == "fit"

    def _check_noise_fit_used(self):
        if self.noise_fit is not None and not self._needs_fit():
            raise ValueError("noise_fit is used only by noise_weights='fit' and baseline_prior={'knee': 'fit'}: neither is set")

    def _fit_noise(self, ctx, signal, tod):
        """The noise law fitted to the Welch spectrum of every row of the signal the mapper bins; the fit range inside
        the pass band of a configured 'filter' pre-processing step."""
        cfg = self.noise_fit or {}
        t = np.asarray(tod.coords.t, float)
        fs = (t.size - 1) / (t[-1] - t[0])
        f, psd = noise_estimate.welch(signal, fs, nperseg=cfg.get("nperseg"), ctx=ctx)
        f_min, f_max = cfg.get("f_min"), cfg.get("f_max")
        band = self.tod_preprocessing.get("filter")
        if band:
            f_np = f.cpu().numpy()
            lo, hi = band.get("f_lower"), band.get("f_upper")
            if lo is not None and lo > 0:
                f_min = max(float(f_np[1]) if f_min is None else f_min, float(lo))
            if hi is not None and hi > 0:
                f_max = min(0.9 * float(f_np[-1]) if f_max is None else f_max, float(hi))
        return noise_estimate.fit_noise(f, psd, f_min=f_min, f_max=f_max, n_bins=cfg.get("n_bins", 32))

    def _det_weight(self, signal, fit=None):
        if isinstance(self.noise_weights, str):
            if self.noise_weights == "uniform":
                return None
            if self.noise_weights == "fit":  # 1 / sigma^2 of the fitted white level; a failed fit weighs 0
                var = fit["sigma"] ** 2
                return torch.where(torch.isfinite(var) & (var > 0), 1.0 / var, torch.zeros_like(var)).contiguous()
            var = signal.double().var(dim=1)
            return torch.where(var > 0, 1.0 / var, torch.zeros_like(var)).contiguous()
        return torch.as_tensor(self.noise_weights).to(self.device)

    def _assemble(self, ctx, sky, records=True):
        """rhs, the binning's scratch weight plane and the blocks of P^T W P over the TODs, and per TOD with detectors (if
        ``records``) its record: ``inputs`` (the ``TodInputs``), ``shape`` (D, T), the operators' arguments ``point`` and
        ``wargs`` (the sample weight, its stride, ``det_w``), ``pre`` (with ``filter_aware`` the pre-processing operator F,
        else None) and what ``_tod_weights`` sets."""
        dev = self.device
        S, Cn = len(self.stokes), len(self.nu)
        shape = (S, Cn, self.n_eta, self.n_xi)
        rhs = torch.zeros(shape, dtype=torch.float64, device=dev)
        scratch = torch.zeros_like(rhs)  # (the binning's |P| weight: not used here)
        blocks = torch.zeros((S * (S + 1) // 2, Cn, self.n_eta, self.n_xi), dtype=torch.float64, device=dev)
        recs = []
        self.noise_fits = []
        for tod in self.tods:
            if tod.dets.n == 0:
                continue
            # a TOD in K_RJ is calibrated per detector to a unit response to I (TOD.to divides by the Mueller [0, 0]
            # element): its pointing matrix carries the Mueller row over that element; in pW the row itself
            inp = self._tod_inputs(tod, ctx, unit_i_response=self.units == "K_RJ", with_operator=self.filter_aware)
            inp, pre = inp if self.filter_aware else (inp, None)
            rec = SimpleNamespace(inputs=inp, shape=inp.shape, point=inp.point, fit=None, det_w=None, pre=pre)
            self._tod_weights(ctx, sky, tod, rec, rhs, scratch)
            if rec.fit is not None:
                self.noise_fits.append(rec.fit)
            rec.wargs = (ptr(inp.weight), 0 if inp.weight is None else inp.weight.stride(0), ptr(rec.det_w))
            ctx.call("mrx_bin_map_blocks", C.byref(sky), *rec.wargs, *rec.point, ptr(blocks))
            if records:
                recs.append(rec)
        return rhs, scratch, blocks, recs

    def _tod_weights(self, ctx, sky, tod, rec, rhs, scratch):
        """``_assemble``'s step that depends on the noise model: the TOD's detector weight ``rec.det_w`` (with ``rec.fit``,
        the noise law fitted for it, if any) and its share of rhs.  Here W of ``noise_weights`` and P^T W d."""
        signal, weight = rec.inputs.signal, rec.inputs.weight
        self._white_weight(ctx, tod, rec)
        # b = P^T W d: the binning's sum, the per-detector weight folded into the sample weight
        w_bin = weight
        if rec.det_w is not None:
            w_bin = (rec.det_w[:, None] * (1.0 if weight is None else weight.double())).float().expand(rec.shape).contiguous()
        bin_map(ctx, sky, rec.inputs._replace(weight=w_bin), rhs, scratch)

    def _white_weight(self, ctx, tod, rec):
        """W of ``noise_weights``: ``rec.det_w`` and, for "fit", ``rec.fit``."""
        if self._needs_fit():
            rec.fit = self._fit_noise(ctx, rec.inputs.signal, tod)
        rec.det_w = self._det_weight(rec.inputs.signal, rec.fit)

    def _solve(self, ctx, blocks, rhs, normal=None):
        """(x, mask, |r| / |b| per iteration, converged): x = H^-1 rhs per pixel, NaN where the block is not solved (mask
        False); with ``normal`` (v -> P^T N^-1 P v) conjugate gradients on the solved pixels, preconditioned by the block
        diagonal, from the block solve."""
        x, mask = self._block_solve(ctx, blocks, rhs, True)
        residuals, converged = [], True
        if normal is not None:
            on_solved = lambda v: torch.where(mask, v, torch.zeros_like(v))  # noqa: E731
            precond = lambda r: self._block_solve(ctx, blocks, r, False)[0]  # noqa: E731
            x, residuals, converged = self._cg(lambda v: on_solved(normal(v)), precond, on_solved(rhs))
        return torch.where(mask, x, torch.full_like(x, float("nan"))), mask, residuals, converged

    def _finish(self, x, blocks, rhs, residuals, converged, **extra):
        """The products every GLS mapper gives (and ``extra``), on the host, and the map."""
        torch.cuda.current_stream(self.device).synchronize()
        data = x.cpu().numpy()
        self.products = {"data": data, "weight": blocks[:1].cpu().numpy(),  # H[0, 0]: [1, C, eta, xi]
                         "blocks": blocks.cpu().numpy(), "rhs": rhs.cpu().numpy(), "residuals": np.asarray(residuals, float),
                         "n_iter": max(len(residuals) - 1, 0), "converged": bool(converged), **extra}
        if self.noise_fits:
            self.products["noise"] = [{k: v.cpu().numpy() for k, v in fit.items() if k in ("white", "knee", "alpha", "sigma")}
                                      for fit in self.noise_fits]
        return self._projection_map(data, self.products["weight"])

    def _block_solve(self, ctx, blocks, r, nan_invalid):
        """z = H^-1 r per pixel and channel; the mask [S, C, eta, xi] (bool, one plane repeated) of the solved blocks."""
        S, Cn = r.shape[:2]
        z = torch.empty_like(r)
        mask = torch.empty((Cn, self.n_eta, self.n_xi), dtype=torch.uint8, device=r.device)
        ctx.call("mrx_map_block_solve", S, Cn, self.n_eta * self.n_xi, ptr(blocks), ptr(r), self.rcond, 1 if nan_invalid else 0,
                 ptr(z), ptr(mask))
        return z, mask.bool().unsqueeze(0).expand(r.shape)

    def _work(self, ctx, sky, recs):
        """The routed operators' work buffer for the TODs of these records, by their [D, T] shapes (None: the atomic form)."""
        need = 0
        for rec in recs:
            lo, full = C.c_size_t(), C.c_size_t()
            if ctx.lib.mrx_map_normal_work_bytes(C.byref(sky), *rec.shape, C.byref(lo), C.byref(full)) == 0:
                need = max(need, _work_bytes(lo.value, full.value, self.device))
        return torch.empty(need, dtype=torch.uint8, device=self.device) if need else None

    def _cg(self, apply, precond, b):
        """Preconditioned conjugate gradients for apply(x) = b from x = precond(b); (x, |r| / |b| per iteration, converged)."""
        b_norm = float(torch.linalg.vector_norm(b)) or 1.0
        x = precond(b)
        r = b - apply(x)
        z = precond(r)
        p = z.clone()
        rz = float(torch.sum(r * z))
        residuals = [float(torch.linalg.vector_norm(r)) / b_norm]
        while residuals[-1] >= self.tol and len(residuals) <= self.max_iter:
            Ap = apply(p)
            alpha = rz / float(torch.sum(p * Ap))
            x.add_(p, alpha=alpha)
            r.sub_(Ap, alpha=alpha)
            residuals.append(float(torch.linalg.vector_norm(r)) / b_norm)
            if residuals[-1] < self.tol:
                break
            z = precond(r)
            rz_new = float(torch.sum(r * z))
            p = z + (rz_new / rz) * p
            rz = rz_new
        converged = residuals[-1] < self.tol
        if not converged:
            logger.warning("%s: conjugate gradients stopped at |r|/|b| = %.3e after %d iterations (tol %.1e)", type(self).__name__,
                           residuals[-1], len(residuals) - 1, self.tol)
        return x, residuals, converged


class MaximumLikelihoodMapper(_GlsMapper):
    """The white-noise generalised-least-squares map:  m = argmin (d - P m)^T W (d - P m),  i.e. (P^T W P) m = P^T W d,
    with P the binning's Stokes-weighted pointing matrix (signed) and W a per-detector weight (``noise_weights``) times
    the per-sample weight of the TOD pre-processing.  I, Q and U are solved jointly: nearest-pixel pointing makes P^T W P
    block-diagonal (one S x S block per pixel and channel) and the map is the exact per-pixel solve; bilinear pointing is
    solved by conjugate gradients preconditioned with those blocks, from the block solve, applying P^T W P on the device
    (``mrx_map_normal_apply``) once per TOD and iteration.  A pixel whose block is singular or has a reciprocal condition
    number below ``rcond`` (unobserved, or seen at one polarisation angle) is left out and is NaN in the map.

    The reference's class name with BinMapper's grid keywords, plus ``noise_weights`` ("inverse_variance": 1 / var of
    each pre-processed detector row; "uniform"; "fit": 1 / sigma^2 of the white level fitted to each pre-processed
    row's Welch spectrum, maria_amd/noise_estimate.py, 0 where the fit fails; or an [ndet] array), ``max_iter``, ``tol``
    (on |r| / |b|), ``rcond`` and ``noise_fit`` (``{"nperseg", "f_min", "f_max", "n_bins"}`` for "fit"; a configured
    'filter' step keeps the fit range inside its pass band).  With "fit" ``products["noise"]`` holds, per TOD, the
    fitted ``white``, ``knee``, ``alpha`` and ``sigma`` (numpy arrays).
    Not converging is not an error: ``products["converged"]`` is False and a warning goes to the "maria" logger.

    ``noise_model`` replaces W by a stationary inverse-noise filter per detector, the GLS map under
    correlated (1/f) noise:  (P^T N^-1 P) m = P^T N^-1 d,  N^-1 = diag(s) K_d diag(s),  K_d the Toeplitz section of the
    lags of maria_amd/noise_filter.py for the detector's law P(f) = white (1 + (knee / f)^alpha) and s the square root of
    the pre-processing's per-sample weight.  "fit" fits the law to every pre-processed row (``noise_fit`` configures it);
    a dict ``{"white", "knee", "alpha"}`` gives it (scalars or [ndet] arrays; knee 0 is white noise, alpha is then not
    needed).  ``noise_filter_length`` (seconds) sets the kernel's half length K = round(length fs) <= 2048 samples
    (default min(2048, T - 1)).  The map is solved by conjugate gradients with nearest and bilinear pointing alike (N^-1
    couples pixels), preconditioned by the block diagonal of P^T diag(s^2 k_d[0]) P.  N^-1 carries the detector weight:
    ``noise_weights`` must keep its default.  ``products["noise_filter"]`` holds per TOD ``K`` and the [D, K + 1]
    ``lags``; with "fit" ``products["noise"]`` the fitted laws.

    Noise shared across detectors: N = (S A S)^-1 + U C U^T, m <= 16 stationary 1/f modes that detector d
    sees with the constant weight U[d, j] (maria_amd/noise_modes.py).  ``noise_modes=m`` with noise_model="fit" fits
    them to every TOD (the top m eigenvectors of the whitened rows' Gram, the mode laws fitted to their series, the
    detector laws refitted without them); a dict model gives them as ``"modes"`` (a [D, m] coupling in the TOD's units)
    and ``"mode_law"`` (``{"white", "knee", "alpha"}``, scalars or [m] arrays).  Modes need one pre-processing weight row
    shared by every detector.  ``products["noise_modes"]`` holds per TOD ``modes``, ``mode_law``, ``dropped`` (the
    fitted modes whose law failed) and the inner solve's iterations (``inner_iter_max``, ``inner_iter_total``).

    ``filter_aware=True`` solves through ``tod_preprocessing`` instead of binning the filtered TOD:
    m = argmin (F d - F P m)^T W (F d - F P m),  (P^T F^T W F P) m = P^T F^T W F d,  F the linear operator that
    ``process_tod`` applied to this TOD (``tod_processing.preprocess_operator``; ``remove_modes`` frozen at the modes and
    row norms the data gave) and W as above.  Conjugate gradients with nearest and bilinear pointing alike (F couples
    pixels), preconditioned by the blocks of P^T W P, from the block solve.  ``products["filter_aware"]`` is True and
    ``products["preprocessing"]`` holds per TOD the ``steps`` applied and, for remove_modes, ``modes`` (U [D, m]) and
    ``row_norms``.  An empty ``tod_preprocessing`` is F = I, the plain map.  Not with ``noise_model`` or ``noise_modes``.

    ``subscan_filter`` (only with ``filter_aware=True``) puts the subscan polynomial filter in front of those
    steps, F = F_pre F':  F' = I - T A T^t M per (detector, segment), the projector ``subscans.Projector`` rebuilds from
    the TOD's own flags (M = (flags == 0), the mask W uses; turnarounds count only if the TOD flagged them) and applies to
    the data once more.  F' T = 0 under any mask, so F' F = F' for the filter F that ``TOD.filter_subscans`` applied
    on the same segments and order, whatever was flagged then: nothing of that filter's state is needed, and a TOD handed
    over unfiltered gives the same map.  A pair that cannot be fitted is the identity in data and model alike.  This
    marginalises a polynomial baseline per (detector, subscan) inside the solve.  ``"recorded"``: ``order``, ``bounds``,
    ``min_hits`` and ``rcond`` of each TOD's ``metadata["subscans"]`` (ValueError where a TOD has none); a dict of
    ``order`` (3), ``bounds`` (None: ``subscans.find_subscans`` of the boresight azimuth with ``turn_frac``, 0.9),
    ``min_hits`` (8) and ``rcond`` (1e-10); or a list of such entries, one per TOD.  ``products["preprocessing"][i]``
    then has ``steps`` starting with "filter_subscans" and ``subscans``: ``order``, ``bounds`` and the ``unfitted``
    (detector, segment) pairs."""

    def __init__(self, tods, center, width=None, height=None, resolution=None, stokes="IQU", nu=None, frame="ra/dec", units="K_RJ",
                 degrees=True, bilinear=False, tod_preprocessing=None, noise_weights="inverse_variance", max_iter=100, tol=1e-6, rcond=1e-3,
                 device="cuda:0", noise_fit=None, noise_model=None, noise_filter_length=None, noise_modes=None, filter_aware=False,
                 subscan_filter=None):
        if not isinstance(filter_aware, (bool, np.bool_)):
            raise ValueError(f"filter_aware {filter_aware!r}: True or False")
        if filter_aware and (noise_model is not None or noise_modes is not None):
            raise ValueError("filter_aware cannot be set with noise_model or noise_modes: F^T N^-1 F is not built")
        if subscan_filter is not None and not filter_aware:
            raise ValueError("subscan_filter is used only with filter_aware=True: the map is solved through the filter")
        self.filter_aware = bool(filter_aware)
        self._init_grid(tods, center, width, height, resolution, stokes, nu, frame, units, degrees, bilinear, tod_preprocessing, device)
        self._init_gls(stokes, noise_weights, max_iter, tol, rcond, noise_fit)
        self._init_noise_model(noise_model, noise_filter_length)
        self._init_noise_modes(noise_modes)
        self._check_noise_fit_used()
        self._init_subscan_filter(subscan_filter)

    SUBSCAN_KEYS = {"order": 3, "bounds": None, "turn_frac": 0.9, "min_hits": 8, "rcond": 1e-10}  # TOD.filter_subscans' defaults

    def _init_subscan_filter(self, value):
        """``self.subscan_filter``: None, or per TOD the resolved ``order``, ``bounds`` (int32, ascending, clamped to the
        TOD), ``min_hits`` and ``rcond``.  Everything is checked here, on the host."""
        from . import subscans
        from .tod import check_bounds_array

        self.subscan_filter = None
        if value is None:
            return
        entries = list(value) if isinstance(value, (list, tuple)) else [value] * len(self.tods)
        if len(entries) != len(self.tods):
            raise ValueError(f"subscan_filter has {len(entries)} entries; there are {len(self.tods)} TODs")
        specs = []
        for entry, tod in zip(entries, self.tods):
            if isinstance(entry, str):
                if entry != "recorded":
                    raise ValueError(f"subscan_filter '{entry}': 'recorded', a dict of {sorted(self.SUBSCAN_KEYS)} or a list of them")
                meta = (getattr(tod, "metadata", None) or {}).get("subscans")
                if meta is None:
                    raise ValueError("subscan_filter='recorded': a TOD has no metadata['subscans'] (TOD.filter_subscans records it)")
                entry = {k: meta[k] for k in ("order", "bounds", "min_hits", "rcond")}
            elif not isinstance(entry, dict) or set(entry) - set(self.SUBSCAN_KEYS):
                raise ValueError(f"subscan_filter {entry!r}: 'recorded', a dict of {sorted(self.SUBSCAN_KEYS)} or a list of them")
            spec = {**self.SUBSCAN_KEYS, **entry}
            order = spec["order"]
            if isinstance(order, bool) or int(order) != order or not 0 <= int(order) < subscans.MAX_ORDER:
                raise ValueError(f"subscan_filter order {order}: an integer in 0 .. {subscans.MAX_ORDER - 1}")
            min_hits = spec["min_hits"]
            if int(min_hits) != min_hits or int(min_hits) < 0:
                raise ValueError(f"subscan_filter min_hits {min_hits}: an integer >= 0")
            if not 0.0 <= float(spec["rcond"]) < 1.0:
                raise ValueError(f"subscan_filter rcond {spec['rcond']}: in [0, 1)")
            T = int(np.asarray(tod.coords.t).size)
            if spec["bounds"] is None:
                bounds, _ = subscans.find_subscans(tod.coords._baz, spec["turn_frac"])
            else:
                bounds = check_bounds_array(spec["bounds"], T)
            specs.append({"order": int(order), "bounds": np.asarray(bounds, np.int32), "min_hits": int(min_hits), "rcond": float(spec["rcond"])})
        self.subscan_filter = specs

    def _subscan_spec(self, tod):
        if self.subscan_filter is None:
            return None
        return next(spec for spec, t in zip(self.subscan_filter, self.tods) if t is tod)

    def _init_noise_model(self, model, length):
        self.noise_model, self.noise_filter_length = model, length
        self.mode_model = None  # a dict model's (coupling [D, m], mode law)
        if isinstance(model, dict) and ("modes" in model or "mode_law" in model):
            model = dict(model)
            coupling, mode_law = model.pop("modes", None), model.pop("mode_law", None)
            self.mode_model = self._check_mode_model(coupling, mode_law)
        if model is None:
            if length is not None:
                raise ValueError("noise_filter_length is used only with noise_model")
            return
        if not (isinstance(self.noise_weights, str) and self.noise_weights == "inverse_variance"):
            raise ValueError("noise_weights cannot be set with noise_model: the inverse-noise filter carries the detector weight")
        if isinstance(model, str):
            if model != "fit":
                raise ValueError(f"noise_model '{model}': 'fit' or a dict of 'white', 'knee', 'alpha'")
        elif isinstance(model, dict):
            if set(model) - {"white", "knee", "alpha"} or not {"white", "knee"} <= set(model):
                raise ValueError(f"noise_model keys {sorted(model)}: 'white', 'knee' and (for a knee > 0) 'alpha'")
            law = {k: np.asarray(v, np.float64) for k, v in model.items()}
            if "alpha" not in law:
                if np.any(law["knee"] != 0):
                    raise ValueError("noise_model: 'alpha' is needed where the knee is not 0")
                law["alpha"] = np.ones(())
            for k, v in law.items():
                for tod in self.tods:
                    if v.ndim and v.shape != (tod.dets.n,):
                        raise ValueError(f"noise_model['{k}'] has shape {v.shape}; the TOD has {tod.dets.n} detectors")
            self.noise_model = law
        else:
            raise ValueError(f"noise_model {model!r}: 'fit' or a dict of 'white', 'knee', 'alpha'")
        if length is not None and not (np.isfinite(length) and length >= 0):
            raise ValueError(f"noise_filter_length {length!r}: a finite number of seconds >= 0")
        for tod in self.tods:
            self._filter_K(tod)

    def _check_mode_model(self, coupling, mode_law):
        if coupling is None:
            raise ValueError("noise_model: 'mode_law' is used only with 'modes'")
        if mode_law is None:
            raise ValueError("noise_model: 'modes' needs 'mode_law' ({'white', 'knee', 'alpha'})")
        U = np.asarray(coupling, np.float64)
        if U.ndim != 2:
            raise ValueError(f"noise_model['modes'] has shape {U.shape}: [ndet, m]")
        m = U.shape[1]
        for tod in self.tods:
            if U.shape[0] != tod.dets.n:
                raise ValueError(f"noise_model['modes'] has shape {U.shape}; the TOD has {tod.dets.n} detectors")
        self._check_mode_count(m)
        if not np.all(np.isfinite(U)):
            raise ValueError("noise_model['modes'] must be finite")
        if not isinstance(mode_law, dict) or set(mode_law) - {"white", "knee", "alpha"} or not {"white", "knee"} <= set(mode_law):
            raise ValueError(f"noise_model['mode_law'] {mode_law!r}: a dict of 'white', 'knee' and (for a knee > 0) 'alpha'")
        law = {k: np.asarray(v, np.float64) for k, v in mode_law.items()}
        if "alpha" not in law:
            if np.any(law["knee"] != 0):
                raise ValueError("noise_model['mode_law']: 'alpha' is needed where the knee is not 0")
            law["alpha"] = np.ones(())
        for k, v in law.items():
            if v.ndim and v.shape != (m,):
                raise ValueError(f"noise_model['mode_law']['{k}'] has shape {v.shape}; there are {m} modes")
        return U, law

    def _check_mode_count(self, m):
        if not 1 <= m <= noise_modes.MAX_MODES:
            raise ValueError(f"{m} noise modes: 1 .. {noise_modes.MAX_MODES}")
        for tod in self.tods:
            if tod.dets.n and m >= tod.dets.n:
                raise ValueError(f"{m} noise modes for a TOD of {tod.dets.n} detectors: fewer modes than detectors")

    def _init_noise_modes(self, modes):
        self.noise_modes = modes
        if modes is None:
            return
        if self.noise_model is None:
            raise ValueError("noise_modes is used only with noise_model='fit'")
        if self.mode_model is not None:
            raise ValueError("noise_modes fits the modes; the noise_model dict gives them ('modes'): not both")
        if not (isinstance(self.noise_model, str) and self.noise_model == "fit"):
            raise ValueError("noise_modes is used only with noise_model='fit' (a dict gives the modes as 'modes' and 'mode_law')")
        if isinstance(modes, bool) or not isinstance(modes, (int, np.integer)):
            raise ValueError(f"noise_modes {modes!r}: an integer number of modes")
        self._check_mode_count(int(modes))
        self.noise_modes = int(modes)

    def _filter_K(self, tod):
        T = tod.coords.t.size
        if self.noise_filter_length is None:
            return noise_filter.default_K(T)
        K = int(round(self.noise_filter_length * self._fs(tod)))
        if not 0 <= K <= noise_filter.MAX_LAG:
            raise ValueError(f"noise_filter_length {self.noise_filter_length} s is {K} samples at {self._fs(tod):.6g} Hz: "
                             f"0 .. {noise_filter.MAX_LAG}")
        return K

    @staticmethod
    def _fs(tod):
        t = np.asarray(tod.coords.t, float)
        return (t.size - 1) / (t[-1] - t[0])

    def _needs_fit(self):
        return super()._needs_fit() or (isinstance(self.noise_model, str) and self.noise_model == "fit")

    def run(self):
        ctx = self._context()
        sky = self._sky()
        if self.noise_model is not None or self.filter_aware:
            return self._run_filtered(ctx, sky)
        # per TOD (bilinear): the normal operator's arguments
        rhs, _, blocks, ops = self._assemble(ctx, sky, records=self.bilinear)
        normal = None
        if ops:
            work = self._work(ctx, sky, ops)

            def normal(v):  # P^T W P v
                y = torch.zeros_like(v)
                for op in ops:
                    ctx.call("mrx_map_normal_apply", C.byref(sky), ptr(v), *op.wargs, *op.point, ptr(y), ptr(work),
                             0 if work is None else work.numel())
                return y

        x, _, residuals, converged = self._solve(ctx, blocks, rhs, normal)
        return self._finish(x, blocks, rhs, residuals, converged)

    def _tod_weights(self, ctx, sky, tod, rec, rhs, scratch):
        """Without ``noise_model`` the white step, and the signal let go.  With it N^-1: ``rec.K``, ``rec.lag``, ``rec.sqrt_w``
        (the window's root), the mode model ``rec.modes`` (``rec.mode_product``: what the products report of it) and
        det_w = k_d[0]; b = P^T N^-1 d follows in ``_run_filtered``, through the buffers the TODs share."""
        if self.filter_aware:  # W as in the white step; b = P^T F^T W F d follows in ``_run_filtered``
            self._white_weight(ctx, tod, rec)
            rec.modes = None
            return
        if self.noise_model is None:
            super()._tod_weights(ctx, sky, tod, rec, rhs, scratch)
            rec.inputs = rec.inputs._replace(signal=None)
            return
        dev = self.device
        signal, weight = rec.inputs.signal, rec.inputs.weight
        D, T = rec.shape
        U = mode_law = None
        dropped = np.zeros(0, np.int64)
        if self._needs_fit() and self.noise_modes:
            fitted = noise_modes.fit(ctx, signal, self.noise_modes, lambda rows: self._fit_noise(ctx, rows, tod))
            rec.fit, U, mode_law, dropped = fitted["law"], fitted["modes"], fitted["mode_law"], fitted["dropped"]
        elif self._needs_fit():
            rec.fit = self._fit_noise(ctx, signal, tod)
        elif self.mode_model is not None:
            U = torch.as_tensor(self.mode_model[0]).to(dev)
            mode_law = self.mode_model[1]
        law = rec.fit or self.noise_model  # the fitted law, else the given one
        K = self._filter_K(tod)
        lag = noise_filter.lags(law["white"], law["knee"], law["alpha"], self._fs(tod), K, device=dev)
        if lag.shape[0] == 1:
            lag = lag.expand(D, -1)
        lag = lag.contiguous()
        sqrt_w = None
        if weight is not None:  # the pre-processing's window: one row shared by every detector, as a rule
            sqrt_w = weight[0].sqrt().contiguous() if bool((weight == weight[:1]).all()) else weight.sqrt()
        model = rec.mode_product = None
        if U is not None:
            if sqrt_w is not None and sqrt_w.dim() == 2:
                raise ValueError("noise modes need one pre-processing weight row shared by every detector; this TOD's differ by row")
            if U.shape[1]:
                beta = noise_modes.mode_lags(mode_law, self._fs(tod), K, device=dev)
                if beta.shape[0] == 1:
                    beta = beta.expand(U.shape[1], -1)
                model = noise_modes.ModeModel(U, beta.contiguous(), lag, sqrt_w, T, noise_modes.inner_tol(self.tol))
            rec.mode_product = {"modes": U, "mode_law": mode_law, "dropped": dropped, "model": model}
        rec.K, rec.lag, rec.sqrt_w, rec.modes = K, lag, sqrt_w, model
        rec.det_w = lag[:, 0].contiguous()

    def _run_filtered(self, ctx, sky):
        """The GLS map under the stationary noise model: b = P^T N^-1 d, then conjugate gradients on the solved pixels with
        the operator project -> filter (in place in one float32 TOD, sized for the largest) -> routed binning.
        With ``filter_aware`` the same loop with F^T W F in the middle: b = P^T F^T W (F d), F d the pre-processed signal,
        and project -> F -> W -> F^T -> routed binning."""
        dev = self.device
        rhs, wgt, blocks, ops = self._assemble(ctx, sky)
        work = self._work(ctx, sky, ops)
        size = lambda op: op.shape[0] * op.shape[1]  # noqa: E731
        tod_buf = torch.empty(max([size(op) for op in ops], default=0), dtype=torch.float32, device=dev)
        # the modes' second TOD, z = A' x of step 1 (noise_modes.apply)
        mode_buf = torch.empty(max([size(op) for op in ops if op.modes is not None], default=0), dtype=torch.float32, device=dev)

        def inv_noise(x, buf, op):  # buf = N^-1 x (buf may be x); filter-aware: buf = F^T W x
            if self.filter_aware:
                if op.det_w is not None:
                    torch.mul(x, op.det_w.float()[:, None], out=buf)
                elif buf is not x:
                    buf.copy_(x)
                if op.inputs.weight is not None:
                    buf.mul_(op.inputs.weight)
                op.pre.apply_transpose(buf)
            elif op.modes is None:
                noise_filter.apply(ctx, x, op.lag, op.sqrt_w, out=buf)
            else:
                noise_modes.apply(ctx, x, op.lag, op.sqrt_w, op.modes, out=buf, scratch=mode_buf[: size(op)].view(op.shape))

        def bin_into(y, buf, op):  # y += P^T buf
            args = (C.byref(sky), ptr(buf), op.shape[1], None, 0, *op.point, ptr(y), ptr(wgt))
            if work is None:
                ctx.call("mrx_bin_map", *args)
            else:
                ctx.call("mrx_bin_map_bucketed", *args, ptr(work), work.numel())

        for op in ops:  # b = P^T N^-1 d
            buf = tod_buf[: size(op)].view(op.shape)
            inv_noise(op.inputs.signal, buf, op)
            bin_into(rhs, buf, op)
            op.inputs = op.inputs._replace(signal=None)  # the signal is not needed any more

        def normal(v):  # P^T N^-1 P v
            y = torch.zeros_like(v)
            for op in ops:
                buf = tod_buf[: size(op)].view(op.shape)
                ctx.call("mrx_map_project", C.byref(sky), ptr(v), *op.point, 1.0, 0.0, ptr(buf), op.shape[1])
                if self.filter_aware:
                    op.pre.apply(buf)
                inv_noise(buf, buf, op)
                bin_into(y, buf, op)
            return y

        x, _, residuals, converged = self._solve(ctx, blocks, rhs, normal if ops else None)
        if self.filter_aware:
            return self._finish(x, blocks, rhs, residuals, converged, filter_aware=True, preprocessing=[op.pre.product() for op in ops])
        extra = {"noise_filter": [{"K": op.K, "lags": op.lag.cpu().numpy()} for op in ops]}
        if any(op.mode_product for op in ops):
            extra["noise_modes"] = [self._mode_product(op.mode_product) for op in ops if op.mode_product]
        return self._finish(x, blocks, rhs, residuals, converged, **extra)

    @staticmethod
    def _mode_product(p):
        as_np = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)  # noqa: E731
        its = p["model"].inner.iterations if p["model"] is not None else []
        return {"modes": as_np(p["modes"]), "mode_law": {k: as_np(v) for k, v in p["mode_law"].items()}, "dropped": as_np(p["dropped"]),
                "inner_iter_max": max(its, default=0), "inner_iter_total": int(sum(its))}


class DestripingMapper(_GlsMapper):
    """The destriped map (the Madam / Keihanen--Kurki-Suonio formulation without a baseline prior): per TOD
    d = P m + F a + n, with F expanding one offset a[d][b] per detector and baseline of ``baseline_length`` seconds
    (L samples; the last baseline of a TOD may be shorter) and n white.  The offsets are the solution of

        A a = F^T W mu (d - P m0),   A a = F^T W mu F a - F^T W mu P M^-1 P^T W F a,   M = P^T W P,

    with m0 = M^-1 P^T W d the white-noise map of ``MaximumLikelihoodMapper`` and mu the mask of the solved pixels (a sample
    in a pixel whose block is not solved takes no part), by conjugate gradients over every TOD's offsets preconditioned by
    1 / hits, hits = F^T W mu 1 (offsets with no hits stay 0).  The map is m = m0 - M^-1 P^T W F a, NaN in unsolved pixels.

    Gauge: a detector's Stokes weights w_k(d) are constant in time, so adding c w_k(d) to the offsets of every detector of
    one map channel and subtracting c from that channel's plane k leaves the data unchanged, for each plane (for I,
    w_I = 1 in K_RJ: a constant on every offset).  A is singular along these S directions per channel; the system is
    consistent and CG converges.  After the solve the offsets of each channel are made hits-orthogonal to them,
    sum hits w_k(d) a = 0 for every k (in K_RJ with I: the hits-weighted mean of the offsets is 0), and the map is formed
    from them: each plane is the sky's up to one constant per channel, which the data cannot determine.

    Operators on the device, no TOD-sized intermediate per iteration: ``mrx_bin_map_baselines`` (P^T W F a),
    ``mrx_map_block_solve`` (M^-1) and ``mrx_baseline_reduce`` (F^T W mu (d - alpha P x), and the hits); F^T W mu F a is
    hits times a.  Nearest-pixel pointing only.  MaximumLikelihoodMapper's keywords plus ``baseline_length`` (seconds; at
    least 16 samples).  ``products`` adds ``baselines`` and ``hits``, one [ndet, nb] array per TOD.

    ``baseline_prior``: None (the above), or ``{"knee": Hz, "alpha": 1.0, "band": 16}`` -- a 1/f prior on the
    offsets, Madam's C_a, from the simulator's noise law: white plus pink, pink equal to white at the knee, slope alpha in
    (0, 2] (maria_amd/destripe_prior.py).  ``knee`` is a scalar or one value per detector of each TOD.  Per TOD and
    detector C_a^-1 = s_d T, T a weighted graph Laplacian over the detector's baselines (K <= 64 signed lags of the inverse
    covariance of L-sample means), s_d = W_d / knee_d^alpha with W_d the detector weight of ``noise_weights``; then

        A a = hits a - F^T W mu P M^-1 P^T W F a + S T a,

    the first and last terms in one ``mrx_baseline_prior_apply``.  With "inverse_variance" W_d is 1 / var of the whole row,
    white and 1/f together, so the prior is weaker than the true one where the 1/f part is large; "fit" takes the
    fitted white level, the prior's own.  The preconditioner is
    (diag(hits) + S T_Kp)^-1, T_Kp the Laplacian of the first ``band`` <= 16 lags (fewer if their symbol goes negative, or
    if the factor, D nb (Kp + 1) 8 bytes a TOD, does not fit in half the free memory; Kp = 0 is the diagonal), factored
    once per ``run()`` (``mrx_baseline_band_factor``, ``mrx_baseline_band_solve``); a detector the band cannot factor (no
    hits, a pivot <= 0) takes 1 / (hits + s_d diag T).  The prior determines offsets with no hits from their neighbours, so
    the gauge shift applies to every baseline of a detector with any hit.  ``products["prior"]``: per TOD K, Kp and the
    weights.

    ``{"knee": "fit"}`` takes each detector's knee from the noise law fitted to its row (``noise_weights="fit"``'s fit,
    ``noise_fit`` its settings) and alpha as the median fitted slope unless ``"alpha"`` is given (``"alpha": "fit"`` is
    the same as leaving it out); the lag table stays shared by all detectors.  ``products["noise"]`` then holds the fits."""

    def __init__(self, tods, center, width=None, height=None, resolution=None, stokes="IQU", nu=None, frame="ra/dec", units="K_RJ",
                 degrees=True, bilinear=False, tod_preprocessing=None, noise_weights="inverse_variance", max_iter=100, tol=1e-6, rcond=1e-3,
                 baseline_length=1.0, baseline_prior=None, device="cuda:0", noise_fit=None):
        if bilinear:
            raise NotImplementedError("DestripingMapper takes nearest-pixel pointing only (bilinear=False)")
        self._init_grid(tods, center, width, height, resolution, stokes, nu, frame, units, degrees, bilinear, tod_preprocessing, device)
        self._init_gls(stokes, noise_weights, max_iter, tol, rcond, noise_fit)
        self.baseline_length = float(baseline_length)
        self.baseline_samples = []  # L per TOD with detectors
        self.sample_rates = []  # fs per TOD with detectors
        for tod in self.tods:
            if tod.dets.n == 0:
                continue
            t = np.asarray(tod.coords.t, float)
            span = t[-1] - t[0] if t.size > 1 else 0.0
            L = round(self.baseline_length * (t.size - 1) / span) if span > 0 else 1 << 30  # (one sample: one baseline)
            if L < 16:
                raise ValueError(f"baseline_length {self.baseline_length} s is {L} samples at this TOD's sample rate: at least 16")
            self.baseline_samples.append(int(min(L, 1 << 30)))
            self.sample_rates.append((t.size - 1) / span if span > 0 else 1.0)
        self.baseline_prior = self._check_prior(baseline_prior)
        self._check_noise_fit_used()

    def _needs_fit(self):
        return super()._needs_fit() or (self.baseline_prior is not None and self.baseline_prior["knee"] == "fit")

    def _check_prior(self, prior):
        """The ``baseline_prior`` keyword, checked: None or {"knee": [ndet] per TOD with detectors, or "fit", "alpha",
        "band"}."""
        if prior is None:
            return None
        if not isinstance(prior, dict) or set(prior) - {"knee", "alpha", "band"} or "knee" not in prior:
            raise ValueError(f"baseline_prior {prior!r}: a dict with 'knee' and optionally 'alpha', 'band'")
        fit = isinstance(prior["knee"], str)
        if fit and prior["knee"] != "fit":
            raise ValueError(f"baseline_prior knee '{prior['knee']}': 'fit', a scalar or one value per detector (Hz)")
        alpha = prior.get("alpha", "fit" if fit else 1.0)
        if isinstance(alpha, str):
            if alpha != "fit":
                raise ValueError(f"baseline_prior alpha '{alpha}': 'fit' or a number in (0, 2]")
            if not fit:
                raise ValueError("baseline_prior alpha 'fit' needs knee 'fit': the slope comes from the same noise fit")
        else:
            alpha = float(alpha)
            if not 0.0 < alpha <= 2.0:
                raise ValueError(f"baseline_prior alpha {alpha}: in (0, 2]")
        band = prior.get("band", 16)
        if int(band) != band or not 0 <= band <= destripe_prior.MAX_BAND:
            raise ValueError(f"baseline_prior band {band}: an integer in 0 .. {destripe_prior.MAX_BAND}")
        if fit:
            return {"knee": "fit", "alpha": alpha, "band": int(band)}
        knee = np.asarray(prior["knee"], float)
        knees = []
        for tod in self.tods:
            if tod.dets.n == 0:
                continue
            if knee.ndim != 0 and knee.shape != (tod.dets.n,):
                raise ValueError(f"baseline_prior knee has shape {knee.shape}: a scalar or one value per detector ({tod.dets.n})")
            k = np.broadcast_to(knee, (tod.dets.n,)).astype(float)
            if not np.all(k > 0) or not np.all(np.isfinite(k)):
                raise ValueError("baseline_prior knee: every value > 0 (Hz)")
            knees.append(k)
        return {"knee": knees, "alpha": alpha, "band": int(band)}

    def run(self):
        dev = self.device
        ctx = self._context()
        sky = self._sky()
        rhs, _, blocks, tods = self._assemble(ctx, sky)
        solve = lambda r: self._block_solve(ctx, blocks, r, False)  # noqa: E731  (0 in unsolved pixels)
        m0, mask = solve(rhs)
        mu = mask[0].to(torch.uint8).contiguous()  # [C, eta, xi]
        # the offsets of all TODs in one vector, [D, nb] views per TOD
        sizes = [(tod.shape[0], -(-tod.shape[1] // L)) for tod, L in zip(tods, self.baseline_samples)]
        offs = np.cumsum([0] + [D * nb for D, nb in sizes])
        views = lambda v: [v[offs[i]:offs[i + 1]].view(sizes[i]) for i in range(len(sizes))]  # noqa: E731
        n = int(offs[-1])
        b, hits = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
        work = self._work(ctx, sky, tods)

        def reduce(i, x, y, h, signal=None):
            ctx.call("mrx_baseline_reduce", C.byref(sky), ptr(signal), 0 if signal is None else signal.stride(0), ptr(x), 1.0,
                     *tods[i].wargs, ptr(mu), self.baseline_samples[i], *tods[i].point, ptr(y), ptr(h))

        def bin_offsets(a):  # P^T W F a
            y = torch.zeros_like(rhs)
            for i, ai in enumerate(views(a)):
                ctx.call("mrx_bin_map_baselines", C.byref(sky), ptr(ai), self.baseline_samples[i], *tods[i].wargs, *tods[i].point, ptr(y),
                         ptr(work), 0 if work is None else work.numel())
            return y

        prior = None

        def apply(a):  # A a = hits a - F^T W mu P M^-1 P^T W F a (+ S T a)
            u = solve(bin_offsets(a))[0]
            if prior is None:
                out = hits * a
            else:
                out = torch.empty_like(a)
                for (D, nb), p, hi, ai, oi in zip(sizes, prior, views(hits), views(a), views(out)):
                    ctx.call("mrx_baseline_prior_apply", D, nb, p["w"].numel(), ptr(p["w"]), ptr(p["scale"]), ptr(hi), ptr(ai), ptr(oi))
            for i, oi in enumerate(views(out)):
                reduce(i, u, oi, None)
            return out

        for i, (bi, hi) in enumerate(zip(views(b), views(hits))):
            reduce(i, m0, bi, hi, signal=tods[i].inputs.signal)  # F^T W mu (d - P m0) and the hits
        if self.baseline_prior is None:
            inv_hits = torch.where(hits > 0, 1.0 / hits, torch.zeros_like(hits))
            precond = lambda r: inv_hits * r  # noqa: E731
        else:
            prior = self._prior_operators(ctx, sizes, views(hits), tods, self._resolved_prior())
            precond = lambda r: self._prior_precond(ctx, sizes, prior, views, r)  # noqa: E731
        a, residuals, converged = self._cg(apply, precond, b)
        self._fix_gauge(a, hits, views, tods)
        x = m0 - solve(bin_offsets(a))[0]
        x = torch.where(mask, x, torch.full_like(x, float("nan")))
        extra = {"baselines": [v.cpu().numpy() for v in views(a)], "hits": [v.cpu().numpy() for v in views(hits)]}
        if prior is not None:
            extra["prior"] = [{"K": p["w"].numel(), "Kp": p["Kp"], "weights": p["w"].cpu().numpy()} for p in prior]
        return self._finish(x, blocks, rhs, residuals, converged, **extra)

    def _resolved_prior(self):
        """baseline_prior with knee "fit" replaced by the fitted knees (a failed fit takes the median of the others) and
        alpha "fit" by the median fitted alpha over every detector of every TOD."""
        cfg = self.baseline_prior
        if cfg["knee"] != "fit":
            return cfg
        alpha = cfg["alpha"]
        if alpha == "fit":
            a = torch.cat([fit["alpha"] for fit in self.noise_fits]).cpu().numpy()
            a = a[np.isfinite(a)]
            alpha = float(np.median(a)) if a.size else 1.0
        knees = []
        for fit in self.noise_fits:
            k = fit["knee"].cpu().numpy()
            ok = np.isfinite(k) & (k > 0)
            knees.append(np.where(ok, k, float(np.median(k[ok])) if ok.any() else 1.0))
        return {"knee": knees, "alpha": alpha, "band": cfg["band"]}

    def _prior_operators(self, ctx, sizes, hits, tods, cfg):
        """Per TOD: the prior's weights and scales on the device, and the preconditioner's band factor (or its diagonal)."""
        out = []
        for i, ((D, nb), hi, tod) in enumerate(zip(sizes, hits, tods)):
            w = destripe_prior.prior_weights(self.sample_rates[i], self.baseline_samples[i], cfg["alpha"], nb)
            det_w = tod.det_w  # the per-detector weight W_d (None: "uniform")
            W = torch.ones(D, dtype=torch.float64, device=self.device) if det_w is None else det_w.double()
            scale = (W / torch.as_tensor(cfg["knee"][i] ** cfg["alpha"]).to(self.device)).contiguous()
            d_w = torch.as_tensor(w).to(self.device)
            diag_T = torch.as_tensor(destripe_prior.laplacian_diagonal(w, nb)).to(self.device)
            diag = hi + scale[:, None] * diag_T[None, :]  # the fall-back: 1 / (hits + s diag T)
            p = {"w": d_w, "scale": scale, "inv_diag": torch.where(diag > 0, 1.0 / diag, torch.zeros_like(diag)), "factor": None}
            Kp = destripe_prior.band_lags(w, cfg["band"])
            while Kp > 0 and D * nb * (Kp + 1) * 8 > torch.cuda.mem_get_info(self.device)[0] // 2:
                Kp -= 1
            p["Kp"] = Kp
            if Kp > 0:
                p["factor"] = torch.empty(D * nb * (Kp + 1), dtype=torch.float64, device=self.device)
                p["ok"] = torch.empty(D, dtype=torch.uint8, device=self.device)
                ctx.call("mrx_baseline_band_factor", D, nb, Kp, ptr(d_w), ptr(scale), ptr(hi), ptr(p["factor"]), ptr(p["ok"]))
                p["inv_diag"].mul_((p["ok"] == 0).double()[:, None])  # the diagonal where the band failed
            out.append(p)
        return out

    def _prior_precond(self, ctx, sizes, prior, views, r):
        """z = (diag(hits) + S T_Kp)^-1 r per TOD (the band solve), 1 / (hits + s diag T) where the band was not factored."""
        z = torch.empty_like(r)
        for (D, nb), p, ri, zi in zip(sizes, prior, views(r), views(z)):
            if p["factor"] is None:
                torch.mul(p["inv_diag"], ri, out=zi)
            else:
                ctx.call("mrx_baseline_band_solve", D, nb, p["Kp"], ptr(p["factor"]), ptr(p["ok"]), ptr(ri), ptr(zi))
                zi.addcmul_(p["inv_diag"], ri)
        return z

    def _fix_gauge(self, a, hits, views, tods):
        """Per map channel, the offsets made hits-orthogonal to the null directions of A, g_k[d][b] = w_k(d) for every
        Stokes plane k:  a -= sum_k c_k g_k  with  G c = n,  G_kl = sum hits g_k g_l,  n_k = sum hits g_k a."""
        S, Cn = len(self.stokes), len(self.nu)
        G = torch.zeros((Cn, S, S), dtype=torch.float64, device=a.device)
        num = torch.zeros((Cn, S), dtype=torch.float64, device=a.device)
        per_tod = []
        for ai, hi, tod in zip(views(a), views(hits), tods):
            sw, d_chan = tod.inputs.stokes_w, tod.inputs.channel.long()
            hs, ha = hi.sum(dim=1), (hi * ai).sum(dim=1)
            G.index_add_(0, d_chan, sw[:, :, None] * sw[:, None, :] * hs[:, None, None])
            num.index_add_(0, d_chan, sw * ha[:, None])
            per_tod.append((sw, d_chan))
        c = (torch.linalg.pinv(G, rtol=1e-12) @ num[:, :, None])[:, :, 0]  # (a channel without hits: G = 0, c = 0)
        for ai, hi, (sw, d_chan) in zip(views(a), views(hits), per_tod):
            shift = (sw * c[d_chan]).sum(dim=1)
            # offsets with no hits stay 0; with a prior they are their neighbours' and move with the detector's others
            seen = hi > 0 if self.baseline_prior is None else (hi > 0).any(dim=1, keepdim=True).expand_as(ai)
            ai.sub_(torch.where(seen, shift[:, None].expand_as(ai), torch.zeros_like(ai)))
