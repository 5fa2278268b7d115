"""Every detector's beam, pointing offset and gain from a scan over a point source (``mrx_tod_source_flag``,
``mrx_tod_beam_normal``).

The offsets (ox, oy) of detector d at sample t from a frame's centre are the float32 numbers the binning computes
(steps 1-3 of the map operators, csrc/mrx_map_pointing.h, composed form).  With the source at (src_x, src_y)(t) from that centre (None: at the centre)
and (u, v) = (ox - src_x, oy - src_y), the model of a row is

    K = 5 (circular):    (A, dx, dy, w, c)          q = w (u^2 + v^2)               w = 1 / sigma^2
    K = 7 (elliptical):  (A, dx, dy, a, b, cc, c)   q = a u^2 + 2 b u v + cc v^2    a quadratic form: no angle
    m = A exp(-q / 2) + c,   r = x - model - m

``source_flags`` marks the samples near (or away from) the source; ``normal_equations`` gives the Gauss-Newton sums
chi2 = sum r^2, JtJ and Jtr of every row over the samples whose flag is 0, in float64 and in a fixed order (the same
inputs give the same bits); ``fit`` is a batched Levenberg-Marquardt on them in float64 torch.  The trial (dx, dy) of
a row go through the binning's pointing code in place of the nominal offsets, rounded to float32: at the optimum the
offsets the fit saw are the bits the binning will see.  The order of the operations is written out in include/mrx.h,
and tests/beamfit_ref.py restates it in numpy."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from ._tod_args import check_like, check_min_hits, check_x
from ._tod_args import context as _context  # under this name the host tests replace it

FWHM_PER_SIGMA = float(np.sqrt(8.0 * np.log(2.0)))


class Normal(NamedTuple):
    """``normal_equations``: ``hits`` [D] int64, ``chi2`` [D], ``JtJ`` [D, K, K] (symmetric), ``Jtr`` [D, K] float64."""

    hits: object
    chi2: object
    JtJ: object
    Jtr: object


class BeamFit(NamedTuple):
    """``fit``: [D] / [D, ..] tensors on the TOD's device.  ``amplitude``, ``dx``, ``dy`` (radians), ``offset`` (the
    constant c); ``fwhm`` (circular: the beam's; elliptical: the geometric mean of the two axes), ``fwhm_major``,
    ``fwhm_minor``, ``angle`` of the major axis from the u axis in (-pi/2, pi/2] (circular: both the fwhm, angle 0);
    ``chi2``, ``hits``; ``cov`` [D, K, K] = (JtJ)^-1 chi2 / (hits - K) in the order of ``params`` [D, K]; ``sigma_dx``,
    ``sigma_dy``; ``ok`` and ``converged`` (bool).  A detector that could not be fitted has NaNs and ok False.
    ``nominal`` [D, 2]: the offsets the fit started from; ``groups`` [D] int64 or None: ``relative_gain``'s default."""

    amplitude: object
    dx: object
    dy: object
    offset: object
    fwhm: object
    fwhm_major: object
    fwhm_minor: object
    angle: object
    chi2: object
    hits: object
    cov: object
    sigma_dx: object
    sigma_dy: object
    ok: object
    converged: object
    params: object
    nominal: object
    groups: object

    def offsets(self):
        """[D, 2] float64 numpy: the fitted (dx, dy), the nominal ones where ``ok`` is false: a detector table's
        ``offsets`` for ``TOD.with_offsets``."""
        import torch

        fitted = torch.stack([self.dx, self.dy], dim=1)
        return torch.where(self.ok[:, None], fitted, self.nominal.to(fitted.device, fitted.dtype)).cpu().numpy()

    def relative_gain(self, groups="band"):
        """[D] float64 numpy, the flat field: the amplitude over the median amplitude of the detector's group's fitted
        detectors; NaN where ``ok`` is false.  ``groups``: "band" (the table's ``band_index``, as ``TOD.fit_beams``
        records it), None (one group) or an integer array."""
        amp, ok = self.amplitude.cpu().numpy(), self.ok.cpu().numpy()
        if isinstance(groups, str):
            if groups != "band" or self.groups is None:
                raise ValueError('groups "band" needs a fit made by TOD.fit_beams; pass None or an integer array')
            g = np.asarray(self.groups.cpu().numpy() if hasattr(self.groups, "cpu") else self.groups, np.int64)
        elif groups is None:
            g = np.zeros(amp.shape[0], np.int64)
        else:
            g = np.asarray(groups)
            if g.shape != amp.shape or g.dtype.kind not in "iu":
                raise ValueError(f"groups must be {amp.shape[0]} integers")
        out = np.full(amp.shape, np.nan)
        for k in np.unique(g):
            sel = (g == k) & ok
            if sel.any():
                out[sel] = amp[sel] / np.median(amp[sel])
        return out


def shape_to_fwhm(a, b, cc):
    """``(fwhm_major, fwhm_minor, angle)`` of the quadratic form q = a u^2 + 2 b u v + cc v^2 (torch tensors): with l the
    eigenvalues of [[a, b], [b, cc]], sigma = 1 / sqrt(l), the major axis belonging to the smaller; the angle of the
    major axis from the u axis in (-pi/2, pi/2].  NaN where the form is not positive definite."""
    import torch

    mean, diff = (a + cc) / 2.0, torch.sqrt(((a - cc) / 2.0) ** 2 + b * b)
    small, big = mean - diff, mean + diff
    nan = torch.full_like(mean, float("nan"))
    good = small > 0
    angle = 0.5 * torch.atan2(-2.0 * b, cc - a)
    angle = torch.where(angle <= -np.pi / 2, angle + np.pi, angle)
    return (torch.where(good, FWHM_PER_SIGMA / torch.sqrt(torch.where(good, small, torch.ones_like(small))), nan),
            torch.where(good, FWHM_PER_SIGMA / torch.sqrt(torch.where(good, big, torch.ones_like(big))), nan), torch.where(good, angle, nan))


def _check_pointing(pointing, like, D, T, need_offsets):
    """(az, el, transform, dx, dy) of a ``mappers.TodInputs`` or anything with those fields (a dict too), on ``like``'s
    device: float32 [T] az and el, float64 [T, 9] transform or None, float32 [D] dx and dy (None where not needed)."""
    import torch

    get = (lambda k: pointing.get(k)) if isinstance(pointing, dict) else (lambda k: getattr(pointing, k, None))
    az, el, transform, dx, dy = (get(k) for k in ("az", "el", "transform", "dx", "dy"))

    def vec(v, name, n, dtype):
        if not isinstance(v, torch.Tensor) or v.dtype != dtype or tuple(v.shape) != (n,) or v.device != like.device or not v.is_contiguous():
            raise ValueError(f"pointing.{name} must be a contiguous [{n}] {str(dtype).split('.')[-1]} tensor on the TOD's device")
        return v

    az, el = vec(az, "az", T, torch.float32), vec(el, "el", T, torch.float32)
    if transform is not None:
        if not isinstance(transform, torch.Tensor) or transform.dtype != torch.float64 or transform.numel() != 9 * T \
                or transform.device != like.device or not transform.is_contiguous():
            raise ValueError(f"pointing.transform must be a contiguous [{T}, 9] float64 tensor on the TOD's device, or None")
    if need_offsets or dx is not None or dy is not None:
        dx, dy = vec(dx, "dx", D, torch.float32), vec(dy, "dy", D, torch.float32)
    return az, el, transform, dx, dy


def _check_center(center):
    try:
        phi, theta = (float(c) for c in center)
    except (TypeError, ValueError):
        raise ValueError("center must be (phi, theta) in radians") from None
    if not (np.isfinite(phi) and np.isfinite(theta)):
        raise ValueError(f"center {center}: two finite angles in radians")
    return phi, theta


def _check_src(src, like, T):
    import torch

    if src is None:
        return None
    if not isinstance(src, torch.Tensor):
        src = torch.as_tensor(np.ascontiguousarray(src, np.float32))
    if tuple(src.shape) != (T, 2):
        raise ValueError(f"src must be [{T}, 2]: the source's offsets from the centre at every sample")
    return src.to(like.device, torch.float32).contiguous()


def source_flags(pointing, center, radius, src=None, inside=True, value=1, flags=None, ctx=None):
    """``flags[d, t] |= value`` where the detector's offset from the source, (u, v), has u^2 + v^2 <= radius^2
    (``inside``) or > radius^2 (not ``inside``); returns the [D, T] uint8 device tensor, ``flags`` updated IN PLACE (any
    row pitch) or a new one.  ``pointing``: a ``mappers.TodInputs`` or the same fields (az, el, transform, dx, dy);
    ``center`` (phi, theta) of the frame and ``radius`` in radians; ``src`` [T, 2] the source's offsets from the centre
    (None: it sits there); ``value`` in 1 .. 255.  The mask is what ``remove_common_mode`` and ``filter_subscans`` take
    as flags so that a bright source does not bias them, and ``fit``'s window is the mask inverted.  Everything
    ``mrx_tod_source_flag`` refuses raises ValueError before any device call."""
    import torch

    from ._lib import ptr

    get = (lambda k: pointing.get(k)) if isinstance(pointing, dict) else (lambda k: getattr(pointing, k, None))
    az, dx = get("az"), get("dx")
    if not isinstance(az, torch.Tensor) or az.dim() != 1 or not isinstance(dx, torch.Tensor) or dx.dim() != 1 or not az.numel() or not dx.numel():
        raise ValueError("pointing needs az [T] and dx [D] tensors with T >= 1 and D >= 1")
    T, D = int(az.shape[0]), int(dx.shape[0])
    if flags is not None:
        if not isinstance(flags, torch.Tensor) or flags.dim() != 2:
            raise ValueError(f"flags must be a [{D}, {T}] uint8 tensor")
        ld_f = check_like(flags, "flags", flags, D, T, "uint8")
    like = az if flags is None else flags
    az, el, transform, dx, dy = _check_pointing(pointing, like, D, T, True)
    phi, theta = _check_center(center)
    radius = float(radius)
    if not (np.isfinite(radius) and radius >= 0):
        raise ValueError(f"radius {radius}: finite and >= 0 (radians)")
    if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= 255:
        raise ValueError(f"value {value}: an integer in 1 .. 255")
    src = _check_src(src, like, T)
    if not like.is_cuda:  # the last refusal: host tensors get every other one first
        raise ValueError("the pointing must be on a device")
    if flags is None:
        flags = torch.zeros((D, T), dtype=torch.uint8, device=like.device)
        ld_f = T
    _context(ctx, flags).call("mrx_tod_source_flag", ptr(az), ptr(el), T, ptr(transform), ptr(dx), ptr(dy), D, phi, theta, ptr(src), radius,
                              1 if inside else 0, int(value), ptr(flags), ld_f)
    return flags


def _check_params(params, like, D):
    import torch

    if not isinstance(params, torch.Tensor):
        params = torch.as_tensor(np.ascontiguousarray(params, np.float64))
    if params.dim() != 2 or params.shape[0] != D or params.shape[1] not in (5, 7) or params.dtype != torch.float64:
        raise ValueError(f"params must be [{D}, 5] (circular) or [{D}, 7] (elliptical) float64")
    return params.to(like.device).contiguous()


def normal_equations(x, pointing, center, params, flags=None, model=None, src=None, ctx=None):
    """``Normal(hits, chi2, JtJ, Jtr)`` of every row of ``x`` ([D, T] float32 device tensor, any row pitch) at the trial
    ``params`` [D, K] float64, over the samples whose ``flags`` ([D, T] uint8, any pitch) are 0; ``model`` [D, T]
    float32 is subtracted from x first.  ``pointing``'s dx, dy are not read (the trial ones stand in their place).
    Everything ``mrx_tod_beam_normal`` refuses raises ValueError before any device call."""
    import ctypes as C

    import torch

    from ._lib import ptr

    D, T, ld_x = check_x(x)
    ld_f = check_like(flags, "flags", x, D, T, "uint8") if flags is not None else 0
    ld_m = check_like(model, "model", x, D, T) if model is not None else 0
    az, el, transform, dx, dy = _check_pointing(pointing, x, D, T, False)
    phi, theta = _check_center(center)
    params = _check_params(params, x, D)
    src = _check_src(src, x, T)
    if not x.is_cuda:
        raise ValueError("x must be a device tensor")
    K = int(params.shape[1])
    nv = 1 + K * (K + 1) // 2 + K
    ctx = _context(ctx, x)
    need = C.c_size_t()
    if ctx.lib.mrx_tod_beam_normal_work_bytes(D, T, K, C.byref(need)) != 0:
        raise ValueError(f"no work size for D {D}, T {T}, K {K}")
    work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty((D, nv), dtype=torch.float64, device=x.device)
    count = torch.empty(D, dtype=torch.int32, device=x.device)
    ctx.call("mrx_tod_beam_normal", ptr(x), ld_x, ptr(model), ld_m, ptr(flags), ld_f, ptr(az), ptr(el), T, ptr(transform), ptr(dx), ptr(dy), D,
             phi, theta, ptr(src), ptr(params), K, ptr(out), ptr(count), ptr(work), work.numel() * 8)
    iu = torch.triu_indices(K, K, device=x.device)
    JtJ = torch.zeros((D, K, K), dtype=torch.float64, device=x.device)
    JtJ[:, iu[0], iu[1]] = out[:, 1:1 + K * (K + 1) // 2]
    JtJ[:, iu[1], iu[0]] = out[:, 1:1 + K * (K + 1) // 2]
    return Normal(count.to(torch.int64), out[:, 0].clone(), JtJ, out[:, 1 + K * (K + 1) // 2:].clone())


def _scales(p):
    """The natural size of a step of every parameter: (|A|, sigma, sigma, shape .., |A|)."""
    import torch

    K = p.shape[1]
    amp = p[:, 0].abs() + 1e-300
    wmax = p[:, 3].abs() if K == 5 else torch.maximum(p[:, 3].abs(), p[:, 5].abs())
    wmax = wmax + 1e-300
    sigma = 1.0 / torch.sqrt(wmax)
    return torch.stack([amp, sigma, sigma] + [wmax] * (K - 4) + [amp], dim=1)


def _positive_shape(p):
    if p.shape[1] == 5:
        return p[:, 3] > 0
    return (p[:, 3] > 0) & (p[:, 5] > 0) & (p[:, 3] * p[:, 5] - p[:, 4] ** 2 > 0)


def fit(x, pointing, center, init, flags, model=None, src=None, elliptical=False, n_iter=20, tol=1e-8, min_hits=16, rcond=1e-12,
        lam0=1e-3, groups=None, ctx=None):
    """``BeamFit`` of every row: a batched Levenberg-Marquardt in float64 torch on ``normal_equations``, from the
    starting point ``init`` ([D, 5]: (A, dx, dy, w, c); with ``elliptical`` the fit runs on (A, dx, dy, w, 0, w, c), or
    ``init`` is [D, 7] itself) over the window ``flags == 0``.  Per detector: (JtJ + lam diag JtJ) step = Jtr, solved as
    ``regress.solve`` does (``rcond``); the step is accepted only if the detector's own chi2 fell (then lam / 10, else
    lam x 10, from ``lam0``); one ``normal_equations`` call an iteration, ``n_iter`` of them; a detector stops moving
    when an accepted step is below ``tol`` of the parameters' natural sizes (|A|, sigma, the shape terms) and its chi2
    fell by less than ``tol`` of itself.  A detector with fewer than max(min_hits, K + 1) samples in the window, a
    singular system or a shape that is not positive definite comes back with NaNs and ``ok`` False, never with an
    exception."""
    import torch

    from . import regress

    D, T, _ = check_x(x)
    if flags is None:
        raise ValueError("flags: the [D, T] uint8 window of the fit (source_flags(..., inside=False))")
    init = _check_params(init, x, D)
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 1:
        raise ValueError(f"n_iter {n_iter}: an integer >= 1")
    if not (np.isfinite(float(tol)) and float(tol) > 0) or not (np.isfinite(float(lam0)) and float(lam0) > 0):
        raise ValueError("tol and lam0: finite and > 0")
    min_hits = check_min_hits(min_hits, allow_bool=False)
    if not 0.0 <= float(rcond) < 1.0:
        raise ValueError(f"rcond {rcond}: in [0, 1)")
    if elliptical and init.shape[1] == 5:
        init = torch.stack([init[:, 0], init[:, 1], init[:, 2], init[:, 3], torch.zeros_like(init[:, 3]), init[:, 3], init[:, 4]], dim=1)
    if not elliptical and init.shape[1] != 5:
        raise ValueError("a [D, 7] init needs elliptical=True")
    K = int(init.shape[1])
    floor = max(min_hits, K + 1)
    ctx = _context(ctx, x) if x.is_cuda else ctx
    az, el, transform, dx0, dy0 = _check_pointing(pointing, x, D, T, False)
    point = {"az": az, "el": el, "transform": transform}
    normal = lambda p: normal_equations(x, point, center, p, flags=flags, model=model, src=src, ctx=ctx)  # noqa: E731
    p = init.clone()
    hits, chi2, JtJ, Jtr = normal(p)
    ok = (hits >= floor) & torch.isfinite(chi2) & torch.isfinite(p).all(dim=1)
    lam = torch.full((D,), float(lam0), dtype=torch.float64, device=x.device)
    done = torch.zeros(D, dtype=torch.bool, device=x.device)
    for _ in range(int(n_iter)):
        active = ok & ~done
        diag = torch.diagonal(JtJ, dim1=1, dim2=2)
        damped = JtJ + torch.diag_embed(lam[:, None] * diag)
        step, solved = regress.solve(torch.where(active[:, None, None], damped, torch.zeros_like(damped)), Jtr, hits, min_hits=floor, rcond=rcond)
        ok = ok & (solved | ~active)
        active = active & solved
        trial = torch.where(active[:, None], p + step, p)
        n2 = normal(trial)
        better = active & (n2.chi2 < chi2) & _positive_shape(trial)
        scale = _scales(p)
        small = (step.abs() <= float(tol) * scale).all(dim=1) & (chi2 - n2.chi2 <= float(tol) * chi2)
        done = done | (better & small) | (active & ~better & (step.abs() <= 1e-3 * float(tol) * scale).all(dim=1))
        p = torch.where(better[:, None], trial, p)
        chi2 = torch.where(better, n2.chi2, chi2)
        JtJ = torch.where(better[:, None, None], n2.JtJ, JtJ)
        Jtr = torch.where(better[:, None], n2.Jtr, Jtr)
        lam = torch.where(better, (lam / 10.0).clamp(min=1e-12), torch.where(active, (lam * 10.0).clamp(max=1e12), lam))
    # cov = (JtJ)^-1 chi2 / (hits - K), by the scaled matrix as regress.solve scales it
    diag = torch.diagonal(JtJ, dim1=1, dim2=2)
    ok = ok & (diag > 0).all(dim=1) & _positive_shape(p)
    s = torch.where(diag > 0, diag, torch.ones_like(diag)).sqrt().reciprocal()
    eye = torch.eye(K, dtype=torch.float64, device=x.device).expand(D, K, K)
    M = torch.where(ok[:, None, None], (JtJ * s[:, :, None]) * s[:, None, :], eye)
    Minv, info = torch.linalg.inv_ex(M)
    ok = ok & (info == 0) & torch.isfinite(Minv).all(dim=2).all(dim=1)
    dof = (hits - K).clamp(min=1).to(torch.float64)
    cov = (Minv * s[:, :, None]) * s[:, None, :] * (chi2 / dof)[:, None, None]
    nan = float("nan")
    p = torch.where(ok[:, None], p, torch.full_like(p, nan))
    cov = torch.where(ok[:, None, None], cov, torch.full_like(cov, nan))
    chi2 = torch.where(ok, chi2, torch.full_like(chi2, nan))
    if K == 5:
        w = p[:, 3]
        major, minor, angle = shape_to_fwhm(w, torch.zeros_like(w), w)
        angle = torch.where(ok, torch.zeros_like(angle), angle)
    else:
        major, minor, angle = shape_to_fwhm(p[:, 3], p[:, 4], p[:, 5])
    nominal = torch.full((D, 2), nan, dtype=torch.float64, device=x.device) if dx0 is None else torch.stack([dx0, dy0], dim=1).to(torch.float64)
    if groups is not None:
        groups = torch.as_tensor(np.asarray(groups, np.int64))
        if tuple(groups.shape) != (D,):
            raise ValueError(f"groups must be {D} integers")
    var = torch.diagonal(cov, dim1=1, dim2=2)
    return BeamFit(p[:, 0], p[:, 1], p[:, 2], p[:, K - 1], torch.sqrt(major * minor), major, minor, angle, chi2, hits, cov, torch.sqrt(var[:, 1]),
                   torch.sqrt(var[:, 2]), ok, ok & done, p, nominal, groups)


# ---- the reference pointing on the host, for tests and demonstrations -----------------------------------------------

def reference_rotations(az, el, transform, center):
    """G [T, 3, 2] float64 with dz = c @ G[t]: steps 1-3 of the map operators composed per sample (mrx_map_pointing.h:
    sample_const), in float64 numpy on the host.  ``transform`` [T, 3, 3] or None; ``center`` (phi, theta) radians."""
    az, el = np.asarray(az, np.float64), np.asarray(el, np.float64)
    a = el - np.pi / 2
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(az), np.sin(az)
    R = np.stack([np.stack([ca * cb, ca * sb, sa], -1), np.stack([-sa * cb, -sa * sb, ca], -1), np.stack([-sb, cb, np.zeros_like(ca)], -1)], axis=1)
    M = np.broadcast_to(np.eye(3), (az.size, 3, 3)) if transform is None else np.asarray(transform, np.float64).reshape(-1, 3, 3)
    phi, theta = _check_center(center)
    P = np.stack([-M[:, :, 0] * np.sin(phi) + M[:, :, 1] * np.cos(phi),
                  (M[:, :, 0] * np.cos(phi) + M[:, :, 1] * np.sin(phi)) * np.sin(theta) - M[:, :, 2] * np.cos(theta)], axis=-1)
    return R @ P


def scan_center(az, el, transform=None):
    """(phi, theta) in radians: the mean direction of the boresight (``az``, ``el`` [T] radians) in the frame that
    ``transform`` [T, 3, 3] rotates into (None: az/el itself), in float64: the default source of ``TOD.mask_source`` and
    ``TOD.fit_beams``."""
    az, el = np.asarray(az, np.float64), np.asarray(el, np.float64)
    xyz = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=-1)
    if transform is not None:
        xyz = np.einsum("tk,tkj->tj", xyz, np.asarray(transform, np.float64).reshape(-1, 3, 3))
    mean = xyz.mean(axis=0)
    mean /= np.linalg.norm(mean)
    return float(np.arctan2(mean[1], mean[0]) % (2 * np.pi)), float(np.arcsin(mean[2]))


def reference_offsets(G, dx, dy):
    """(ox, oy) [D, T] float64 of detectors at (dx, dy) through the rotations ``G`` of ``reference_rotations``."""
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    r = np.hypot(dx, dy)
    s = np.sinc(r / np.pi)
    dz = np.einsum("dk,tkj->dtj", np.stack([-dy * s, np.cos(r), -dx * s], axis=-1), G)
    rr = np.hypot(dz[..., 0], dz[..., 1])
    f = np.where(rr > 0, np.arcsin(np.minimum(rr, 1.0)) / np.where(rr > 0, rr, 1.0), 1.0)
    return -dz[..., 0] * f, -dz[..., 1] * f


def inject_source(data, az, el, transform, center, params, src=None):
    """A float32 copy of the host array ``data`` [D, T] with the model's own source added, m = A exp(-q / 2) + c at the
    per-detector ``params`` [D, 5] or [D, 7] (for tests and demonstrations): computed on the host in float64 from the
    reference pointing at the float32-rounded (dx, dy) of ``params``, as the device takes them, so that ``params`` is
    the exact truth of a fit.  ``az``, ``el`` [T] boresight; ``transform`` [T, 3, 3] or None; ``src`` [T, 2] or None."""
    x = np.array(data, np.float32)
    p = np.asarray(params, np.float64)
    if x.ndim != 2 or p.ndim != 2 or p.shape[0] != x.shape[0] or p.shape[1] not in (5, 7):
        raise ValueError("data must be [D, T] and params [D, 5] or [D, 7]")
    if np.asarray(az).shape != (x.shape[1],) or np.asarray(el).shape != (x.shape[1],):
        raise ValueError(f"az and el must be [{x.shape[1]}]")
    K = p.shape[1]
    G = reference_rotations(az, el, transform, center)
    ox, oy = reference_offsets(G, p[:, 1].astype(np.float32), p[:, 2].astype(np.float32))
    if src is not None:
        src = np.asarray(src, np.float64)
        if src.shape != (x.shape[1], 2):
            raise ValueError(f"src must be [{x.shape[1]}, 2]")
        ox, oy = ox - src[None, :, 0], oy - src[None, :, 1]
    if K == 5:
        q = p[:, 3, None] * (ox * ox + oy * oy)
    else:
        q = p[:, 3, None] * (ox * ox) + 2.0 * p[:, 4, None] * (ox * oy) + p[:, 5, None] * (oy * oy)
    return (x.astype(np.float64) + p[:, 0, None] * np.exp(-q / 2.0) + p[:, K - 1, None]).astype(np.float32)
